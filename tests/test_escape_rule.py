"""CPU test of the walk's escape rule (brickmap_amd/csrc/escape.h): the predicate and the table's definition.

escape.h is plain C++ shared by the device kernels (escape.hip builds the table with it, traverse.h tests rays against it) and
tests/escape_check.cpp, which builds the table of small random worlds pass by pass as the kernels do, compares it with the definition
written out as loops, and walks random rays cell by cell as the reference does: from the first cell in which the predicate holds, the
walk never meets an occupied cell -- for every octant, with zero direction components, starts on cell faces, empty and full worlds, a
single brick in the far corner cell of the quadrant and a ceiling above the start cell.
The same program is built and run a second time under the address and undefined-behaviour sanitizers: host code with its own main.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "escape_check.cpp")


def _run(exe, worlds):
    r = subprocess.run([str(exe), str(worlds)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    words = r.stdout.split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def test_escape_rule_replays_reference_walk(tmp_path):
    exe = tmp_path / "escape_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), SRC])
    n = _run(exe, 300)
    # the run did exercise the rule: rays that escape on the way, rays that escape where they start, rays that never do
    assert n["rays"] > 200_000 and n["cells"] > 4 * n["rays"] and n["tables"] >= 600
    assert n["rays"] // 20 < n["at_start"] < n["escaped"] < n["rays"] - n["rays"] // 20


def test_escape_rule_under_sanitizers(tmp_path):
    exe = tmp_path / "escape_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), SRC])
    n = _run(exe, 60)
    assert n["rays"] > 40_000 and n["tables"] >= 120
