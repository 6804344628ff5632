"""CPU test of the view plane's rule (brickmap_amd/csrc/viewfield.h): the plan of a camera position, the bytes and the 255 stamps.

viewfield.h is plain C++ shared by the device kernel (viewfield.hip builds the tenth plane of the cube field with it) and
tests/view_check.cpp, which builds the plane of small worlds (16^3, 32 x 32 x 16 and 16 x 16 x 32 cells: terrain, a cross of ridges with
one-cell notches, overhangs and floating bricks, a hollow mountain, an empty world) for camera positions at the centre, one cell above
the terrain, inside a notch and inside the hollow, in the top layer, in a corner cell, at integer coordinates and 1e-4 cell from a
face; compares it with the rule written out a second time; and walks at least 10^5 rays from every position cell by cell as the
reference does (fp32 tmax as ray_setup and the move compute it; directions uniform over the sphere, aimed at cell corners and edges,
and with zero components): byte 0 exactly where a cell is occupied, nothing occupied behind a 255 cell, and from a cell of byte n every
cell entered before an axis has moved n cells is empty and inside the grid.  Every class of byte must have been visited in every
world built to have it.  The program also reports the violations found with the margin set to 0: a record that the margin matters.
The same program is built and run a second time under the address and undefined-behaviour sanitizers: host code with its own main.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "view_check.cpp")
PER_POSITION = 100_000


def _run(exe):
    r = subprocess.run([str(exe), str(PER_POSITION)], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    words = r.stdout.split()
    n = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    # fifteen worlds; six positions each, seven where there is a notch or a hollow; seven plans refused
    assert n["planes"] == 9 * 6 + 6 * 7 and n["refused"] == 7
    assert n["rays"] >= n["planes"] * PER_POSITION - n["planes"] * 10  # (a direction that rounds to zero is not a ray)
    # the run did exercise the rule: cells whose byte is longer than their octant's, and many cells per ray
    assert n["longer_bytes"] > 10_000 and n["cells"] > 8 * n["rays"]
    for kind in range(5):
        for dims in ("16x16", "32x16", "16x32"):
            assert n[f"world_{kind}_{dims}_255"] > 0
            assert (n[f"world_{kind}_{dims}_n"] > 0 and n[f"world_{kind}_{dims}_0"] > 0) == (kind != 4)
    print("violations with the margin set to 0:", n["margin0_violations"], "in", n["margin0_rays"], "rays")


def test_view_plane_rule_replays_reference_walk(tmp_path):
    exe = tmp_path / "view_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", str(exe), SRC])
    _run(exe)


def test_view_plane_rule_under_sanitizers(tmp_path):
    exe = tmp_path / "view_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), SRC])
    _run(exe)
