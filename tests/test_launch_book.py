"""tests/launch_book_check.cpp: the host-only book of who waits for whom (csrc/launch_book.h) -- the stream table (a frame's stream against
upload batches, the retirement of a 17th stream, a residency reset) and the rings (the entries a launch of the frame ring takes and the
earlier launches it waits for, the clock slots of the most recent launches, the query ring) -- scripted step by step against answers
written out by hand, in a program with its own main, built plain and under the address and undefined-behaviour sanitizers.  CPU only;
nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "launch_book_check.cpp")
STEPS = 406  # the CHECKs of the seven sequences, loops included


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    assert f"steps {STEPS}\n" in r.stdout, r.stdout


def test_launch_book_program(tmp_path):
    exe = tmp_path / "launch_book_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    _run(exe)


def test_launch_book_program_under_sanitizers(tmp_path):
    exe = tmp_path / "launch_book_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), SRC])
    _run(exe)
