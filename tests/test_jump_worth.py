"""CPU test of the rule "is a jump worth it here" (brickmap_amd/csrc/steps.h: jump_worth, and field_state's use of it).

tests/jump_worth_check.cpp includes steps.h -- the very functions the kernels run -- and checks that jump_worth implies jump_possible on
20 M random and special tmax / tdelta triples (signed zeros, the 1e6 sentinel of a zero direction component, tmax on and next to binade
ends, tdelta from 1 to 1e6, raw bit patterns), that a walk by "single moves while not worth a jump, else jump" is in the state of the
reference's one-cell stepping after every operation (the ray families of tests/jump_check.cpp), and that no walk stays not-worth for
longer than the bound its tdelta gives (30 moves for a unit direction) unless its tmax has left every supported world.
The same program is built and run a second time under the address and undefined-behaviour sanitizers: host code with its own main.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "jump_worth_check.cpp")


def _run(exe, triples, rays):
    r = subprocess.run([str(exe), str(triples), str(rays)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    out = dict(zip(words[0::2], (int(w) for w in words[1::2])))
    assert out["failures"] == 0, r.stdout + r.stderr
    return out


def test_jump_worth_implies_possible_and_walks_replay_reference(tmp_path):
    exe = tmp_path / "jump_worth_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), SRC])
    out = _run(exe, 20_000_000, 200_000)
    # the run did exercise the code: worth and not-worth triples, jumps, rides, single moves, runs of not-worth moves
    assert out["triples"] == 20_000_000 and 1_000_000 < out["worth"] < 19_000_000
    assert out["jumps"] > 1_000_000 and out["rides"] > 100_000 and out["singles"] > 1_000_000
    assert 3 <= out["longest-unit-run"] <= 30


def test_jump_worth_under_sanitizers(tmp_path):
    exe = tmp_path / "jump_worth_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), SRC])
    out = _run(exe, 1_000_000, 20_000)
    assert out["jumps"] > 100_000 and out["singles"] > 100_000
