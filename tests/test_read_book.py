"""tests/read_book_check.cpp: the host-only book of the calls that only read the world (csrc/read_book.h) -- the slabs of a box outside the
world against a per-voxel count (128^3 and 256 x 256 x 128: inside, across every face, an edge, a corner, around the world, outside, empty,
300 seeded boxes), the offsets of a voxel in a pitched volume and in a label volume, every refusal of the label box with edges of up to
2^32 - 1 on one, two and three axes, label_clip against a clip by hand, the patch list of hand-made preloaded and streaming worlds against a
scan of every cell, its layout around the 64-byte line and the 64 KiB it starts with (862 bricks fit, 863 do not) and a round trip out of a
poisoned buffer, every refusal of the two queries with its message, the LoD cell of an origin, and the label clock -- against answers
computed in the program itself, which has its own main and is built plain and under the address and undefined-behaviour sanitizers.
CPU only; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "read_book_check.cpp"), os.path.join(ROOT, "brickmap_amd", "csrc", "world.cpp")]
FLAGS = ["-std=c++17", "-ffp-contract=off"]  # (no contraction: as the library's host code is built)
STEPS = 2839  # the CHECKs of the sequences (a) ... (e), loops included


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    assert f"steps {STEPS}\n" in r.stdout, r.stdout


def test_read_book_program(tmp_path):
    exe = tmp_path / "read_book_check"
    subprocess.check_call(["g++", "-O2", *FLAGS, "-Wall", "-Werror", "-o", str(exe), *SRCS, "-lpthread"])
    _run(exe)


def test_read_book_program_under_sanitizers(tmp_path):
    exe = tmp_path / "read_book_check_san"
    subprocess.check_call(["g++", "-O1", "-g", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), *SRCS, "-lpthread"])
    _run(exe)


def test_read_book_needs_no_hip(tmp_path):
    """the header compiles with a plain host compiler and no ROCm include path"""
    src = tmp_path / "only.cpp"
    src.write_text('#include "read_book.h"\nint main() { return sizeof(bm::PatchList) ? 0 : 1; }\n')
    subprocess.check_call(["g++", *FLAGS, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "brickmap_amd", "csrc"), str(src)])
