"""CPU test of the rule that decides, in the shade block, whether a shadow ray is drawn at all (brickmap_amd/csrc/shadowheight.h shadow_origin).

shadow_origin is plain C++ shared by trace.hip and tests/shadow_origin_check.cpp.  The program checks it against its definition written out a
second time -- 1.2 M origins in worlds of 16^3, 32 x 32 x 16 and 16 x 16 x 32 cells: random interior points, exact multiples of 8 and their fp32
neighbours, 0, the grid's size and height and one ulp either side, negative coordinates, denormals, infinities, NaN -- and then builds a
slice with the functions tests/shadowheight_check.cpp uses (shadowheight_host.h) and walks rays of the cone, cell by cell with the
reference's rounded tmax, from origins the function calls dark: each must start in the cell the function named, below its column's dark
height, and enter a full cell before it leaves the grid.  Built and run plain, and a second time as a stand-alone program under the address
and undefined-behaviour sanitizers (host code with its own main).
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "shadow_origin_check.cpp")
THOUSANDS = 400  # origins per world for the comparison with the definition


def _run(exe):
    r = subprocess.run([str(exe), str(THOUSANDS)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.strip().splitlines()[-1].split()
    n = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    assert n["failures"] == 0 and n["violations"] == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert n["origins"] >= 1_000_000 and n["origins"] == n["decided"] + n["undecided"]
    # both answers are exercised: the hard values make most mixed origins undecided, the interior points decided
    assert n["decided"] > 50_000 and n["undecided"] > 50_000
    # nine slices (three worlds x three suns), each with dark origins, each dark origin's ray walked
    lines = [ln for ln in r.stdout.splitlines() if "origins dark" in ln]
    assert len(lines) == 9 and n["rays"] == n["dark_origins"] > 9 * 1000


def test_shadow_origin_equals_its_definition_and_dark_origins_are_occluded(tmp_path):
    exe = tmp_path / "shadow_origin_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), SRC])
    _run(exe)


def test_shadow_origin_under_sanitizers(tmp_path):
    exe = tmp_path / "shadow_origin_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), SRC])
    _run(exe)
