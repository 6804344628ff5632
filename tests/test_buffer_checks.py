"""tests/buffer_checks_check.cpp: the span-overlap and alignment helpers of csrc/buffer_checks.h -- what every device operator checks a
caller's buffers with -- against brute force, in a program with its own main, built plain and under the address and undefined-behaviour
sanitizers.  CPU only; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "buffer_checks_check.cpp")
SPANS = 41 * 13                    # starts 0 ... 40, lengths 0 ... 12
TOP_SPANS = 17 * 33 + 5 * 5        # within 16 bytes of UINTPTR_MAX with lengths 0 ... 32, and addresses 0 ... 4 with lengths 0 ... 4


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    words = r.stdout.split()
    n = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    assert n["overlap"] == SPANS * SPANS and n["aligned"] == 3 * 64 and n["all_aligned"] == 3 * 64 ** 3 and n["top"] == TOP_SPANS * TOP_SPANS, n
    assert 0 < n["beyond"] < n["top"], "pairs with a span that ends beyond the address space, and pairs without"
    return n


def test_buffer_checks_program(tmp_path):
    exe = tmp_path / "buffer_checks_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), SRC])
    _run(exe)


def test_buffer_checks_program_under_sanitizers(tmp_path):
    exe = tmp_path / "buffer_checks_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), SRC])
    _run(exe)
