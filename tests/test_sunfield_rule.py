"""CPU test of the sun plane's rules (brickmap_amd/csrc/sunfield.h): the plan of a sun, the bytes and the 255 stamps.

sunfield.h is plain C++ shared by the device kernels (sunfield.hip builds the ninth plane of the cube field with it) and
tests/sunfield_check.cpp, which builds the plane of small worlds (16^3, 32 x 32 x 16 and 16 x 16 x 32 cells: random, terrain, terrain
with overhangs, a single floating brick) slab by slab as the kernels do and walks rays of the cone cell by cell as the reference does,
from random points: byte 0 exactly where a cell is occupied, nothing occupied behind a 255 cell, and from a cell of byte n nothing
occupied is entered before an axis has moved n cells.  Suns with each dominant axis, in several octants, a wide cone and a very low
sun; a cone across an octant boundary, a sun below the horizon and a minor slope of 1 must come out "not valid".
The same program is built and run a second time under the address and undefined-behaviour sanitizers: host code with its own main.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sunfield_check.cpp")
PER_SUN = 100_000


def _run(exe):
    r = subprocess.run([str(exe), str(PER_SUN)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    words = r.stdout.split()
    n = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    # seven valid suns x twelve worlds, at least 100 k rays each sun; three suns refused
    assert n["planes"] == 84 and n["invalid"] == 3 and n["rays"] >= 7 * PER_SUN
    # the run did exercise the rules: rays that end at a stamp and rays that never do, bytes long enough for a jump
    assert n["rays"] // 10 < n["stamped"] < n["rays"] - n["rays"] // 10 and n["long_bytes"] > n["rays"] and n["cells"] > 8 * n["rays"]


def test_sun_plane_rules_replay_reference_walk(tmp_path):
    exe = tmp_path / "sunfield_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), SRC])
    _run(exe)


def test_sun_plane_rules_under_sanitizers(tmp_path):
    exe = tmp_path / "sunfield_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), SRC])
    _run(exe)
