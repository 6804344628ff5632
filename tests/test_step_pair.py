"""CPU test of the pair move of the single-move passes (brickmap_amd/csrc/steps.h: step_pair_ahead, step_pair_commit) and of the guard
bytes round the cube field (brickmap_amd/csrc/field_layout.h: field_guard_bytes, the function the allocation uses).

tests/step_pair_check.cpp includes both headers -- the very functions the kernels and the allocation run -- and checks on 20 M states
(random, ties in every pair of axes and in all three, zero direction components, signed zeros, NaN, raw bit patterns) that the pair move
with "stops at cell 1" and with "continues" equals one and two plain moves bit for bit (tmax, cell, last_step), and that the cell it looks
at is the second plain move's whether committed or not; then, for every BASELINE world, a flat and a tall one, with 8, 9 and 10 planes,
that from every cell of the bordered box of the first and the last plane each of the six increments stays inside the guarded allocation.
The same program is built and run a second time under the address and undefined-behaviour sanitizers: host code with its own main.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "step_pair_check.cpp")


def _run(exe, states, largest):
    r = subprocess.run([str(exe), str(states), str(largest)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    out = dict(zip(words[0::2], (int(w) for w in words[1::2])))
    assert out["failures"] == 0, r.stdout + r.stderr
    return out


def test_pair_move_replays_plain_moves_and_stays_inside_the_guards(tmp_path):
    exe = tmp_path / "step_pair_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), SRC])
    out = _run(exe, 20_000_000, 1024)
    # the run did exercise the code: both outcomes, every kind of state, every axis as the second move, every world
    assert out["states"] == 20_000_000 and 3_000_000 < out["stops"] < 7_000_000
    assert min(out["ties2"], out["ties3"], out["zerodir"]) > 2_000_000 and out["nan"] > 500_000 and out["negzero"] > 100_000
    assert min(out["movex"], out["movey"], out["movez"]) > 1_000_000
    assert out["worlds"] == 6 and out["cells"] > 4 * 514 ** 3
    assert out["beyond"] > 0, "some looked-at cell does lie in the guard bytes: the check is not vacuous"


def test_pair_move_under_sanitizers(tmp_path):
    exe = tmp_path / "step_pair_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), SRC])
    out = _run(exe, 1_000_000, 128)
    assert out["worlds"] == 2 and out["stops"] > 100_000 and out["beyond"] > 0
