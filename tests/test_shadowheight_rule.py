"""CPU test of the shadow heights' rule (brickmap_amd/csrc/shadowheight.h): the plan's upper rise, the recurrence of S and the dark heights.

shadowheight.h is plain C++ shared by the device kernels (sunfield.hip builds slice 8 of the escape table with it) and
tests/shadowheight_check.cpp, which builds the dark heights of small worlds (16^3, 32 x 32 x 16 and 16 x 16 x 32 cells: terrain, a cross of
ridges with one-cell notches, overhangs and floating bricks, a hollow mountain, a partly filled top layer, an empty world) slab by slab as
the kernel does, compares them with the definition written out a second time, asserts that no cell stamped 255 by the sun plane is dark,
and walks rays of the cone cell by cell as the reference does from random points of every dark cell: each must enter a full cell before
it leaves the grid or reaches a 255 stamp.  Suns with both horizontal dominant axes, in four octants, a wide cone and a very low sun; a
z-dominant sun and a cone across an octant boundary must yield all-zero slices.  Every world built to cast shadow must end rays.
The same program is built and run a second time under the address and undefined-behaviour sanitizers (host code with its own main), and
twice with the rule loosened on purpose -- the rise's lower bound in place of the upper one, and no margin -- which the walk must catch.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "shadowheight_check.cpp")
PER_CELL = 12


def _counts(r):
    words = r.stdout.strip().splitlines()[-1].split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def _run(exe):
    r = subprocess.run([str(exe), str(PER_CELL)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    n = _counts(r)
    assert n["failures"] == 0 and n["violations"] == 0 and n["barren"] == 0, r.stdout[-2000:] + r.stderr
    # seven suns x three sizes x six worlds; the z-dominant sun and the cone across an octant boundary get zero slices
    assert n["slices"] == 126 and n["zero_slices"] == 36
    # the run did exercise the rule: five suns x three sizes x five worlds that cast shadow, each with rays ended (barren == 0), and many in all
    assert n["dark_cells"] > 100_000 and n["rays_ended"] == PER_CELL * n["dark_cells"]
    lines = [ln for ln in r.stdout.splitlines() if "rays ended" in ln]
    assert len(lines) == 90 and sum(" 0 rays ended" in ln for ln in lines) == 15, "only the empty worlds end no ray"


def test_shadow_height_rule_replays_reference_walk(tmp_path):
    exe = tmp_path / "shadowheight_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), SRC])
    _run(exe)


def test_shadow_height_rule_under_sanitizers(tmp_path):
    exe = tmp_path / "shadowheight_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), SRC])
    _run(exe)


def test_loosened_rules_are_caught(tmp_path):
    """rise_hi replaced by the lower bound `rise` (1), the margin dropped and a cell dark by its floor (2): both must report violations --
    1 240 and 15 770 of 1.4 M / 1.6 M rays at 6 rays per dark cell (profiles/r10_shadow_heights.txt)"""
    for loose in (1, 2):
        exe = tmp_path / f"shadowheight_check_loose{loose}"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", f"-DBM_SHADOWHEIGHT_LOOSE={loose}", "-o", str(exe), SRC])
        r = subprocess.run([str(exe), str(PER_CELL)], capture_output=True, text=True, timeout=600)
        n = _counts(r)
        assert r.returncode != 0 and n["violations"] > 100, r.stdout[-2000:] + r.stderr
