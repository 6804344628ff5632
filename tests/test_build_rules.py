"""csrc/Makefile: once the listings are built, `make asm` has nothing left to do -- a rule that always fires would compile every kernel
file again in every compiled-shape test module (CPU only)."""
import subprocess

from _compiled import CSRC, build_dir


def test_a_second_make_asm_does_nothing():
    build_dir()
    assert subprocess.call(["make", "-q", "-C", CSRC, "asm"]) == 0
