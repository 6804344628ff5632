"""tests/pool_book_check.cpp: the host-only book of which brick is resident where (csrc/pool_book.h) -- the pools of a reset and of a preload,
the slots and the pool growths of a request ring with its one move per pool, stale and impossible ring entries, freed slots, a preloaded edit
on an exact-fit pool, the growth size, a region allocator that fails in the middle of a batch, the two request rings in both modes, and a
seeded script of 3000 mixed steps with the invariants checked after each -- against answers written out by hand, in a program with its own
main, built plain and under the address and undefined-behaviour sanitizers.  CPU only; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pool_book_check.cpp")
STEPS = 3184  # the CHECKs of the sequences (a) ... (j), loops included: 3002 of them are the seeded script's


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    assert f"steps {STEPS}\n" in r.stdout, r.stdout


def test_pool_book_program(tmp_path):
    exe = tmp_path / "pool_book_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    _run(exe)


def test_pool_book_program_under_sanitizers(tmp_path):
    exe = tmp_path / "pool_book_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), SRC])
    _run(exe)
