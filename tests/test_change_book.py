"""tests/change_book_check.cpp: the host-only book of what a change of the host world sends to the device (csrc/change_book.h) -- the supercells
a box reaches against a scan of every voxel, supercell_coords against supercell_id, the words, arena slots and bricks of the touched cells and
the two boxes of the FieldChange after real edits and region writes of hand-made worlds (256 x 256 x 128 and 128^3, preloaded and streaming),
the staging layout with a round trip out of a poisoned buffer, the stage clocks of edits and region writes, and a seeded script of 400 random
edits and region writes whose (cell, word) pairs are replayed into a model index grid -- against answers computed in the program itself, which
has its own main and is built plain and under the address and undefined-behaviour sanitizers.  CPU only; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "change_book_check.cpp"), os.path.join(ROOT, "brickmap_amd", "csrc", "world.cpp")]
STEPS = 1694  # the CHECKs of the sequences (a) ... (f), loops included


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    assert f"steps {STEPS}\n" in r.stdout, r.stdout


def test_change_book_program(tmp_path):
    exe = tmp_path / "change_book_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), *SRCS, "-lpthread"])
    _run(exe)


def test_change_book_program_under_sanitizers(tmp_path):
    exe = tmp_path / "change_book_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), *SRCS, "-lpthread"])
    _run(exe)


def test_change_book_needs_no_hip(tmp_path):
    """the header compiles with a plain host compiler and no ROCm include path"""
    src = tmp_path / "only.cpp"
    src.write_text('#include "change_book.h"\nint main() { return sizeof(bm::CellBatch) ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "brickmap_amd", "csrc"), str(src)])
