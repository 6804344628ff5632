"""tests/field_book_check.cpp: the host-only book of the walk fields (csrc/field_book.h) -- which of the sun plane, its shadow-height slice and
the view plane stands, what makes each stale and what a launch that is about to read one has to build first -- scripted event by event
against decisions and counters written out by hand, in a program with its own main, built plain and under the address and
undefined-behaviour sanitizers.  CPU only; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "field_book_check.cpp")
STEPS = 58  # the CHECKs of the eight sequences


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    assert f"steps {STEPS}\n" in r.stdout, r.stdout


def test_field_book_program(tmp_path):
    exe = tmp_path / "field_book_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    _run(exe)


def test_field_book_program_under_sanitizers(tmp_path):
    exe = tmp_path / "field_book_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), SRC])
    _run(exe)
