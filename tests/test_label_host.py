"""bm_host_label_volume (csrc/label_host.cpp: plain loops over the rules of csrc/label.h) against the numpy model of the labelling
contract (tests/_label_model.py), byte for byte, on seeded volumes and the hand-made shapes -- CPU only.  Where scipy imports, its
labelling must give the same partition.  The component table's definition is pinned on the model's labels.  And tests/label_check.cpp, a
program with its own main that links the host routine alone, built plain and under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import _label_model as model
from _box_cases import world_voxels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLS = (0.1, 0.3, 0.5, 0.9)
# (seed, shape [z, y, x]): odd sizes, one-voxel-thick ones, and the largest the model is meant for
SEEDED = [(s, shp) for s, shp in enumerate([(1, 1, 1), (1, 1, 37), (1, 29, 1), (31, 1, 1), (7, 9, 11), (8, 8, 8), (9, 16, 17), (16, 24, 40), (23, 31, 33)])]


@pytest.fixture(scope="module")
def cube_cut():
    """a 48 x 48 x 96 cut of the "cube" world and the model's labels of it: computed once, left unchanged"""
    cut = world_voxels("cube")[:48, :48, :96]
    labels, count, rounds = model.model_labels(cut)
    assert rounds > 50 and count > 10_000
    return cut, labels, count


@pytest.mark.parametrize("fill", FILLS)
def test_host_routine_equals_the_model_on_seeded_volumes(bm, fill):
    for seed, shp in SEEDED:
        vol = model.seeded_volume(1000 * seed + int(100 * fill), shp, fill)
        want, count, _ = model.model_labels(vol)
        got, n = bm.host_label_volume(vol)
        assert got.dtype == np.int32 and got.shape == vol.shape
        assert n == count and np.array_equal(got, want), (fill, seed, shp)


def test_host_routine_equals_the_model_on_a_cut_of_the_cube_world(bm, cube_cut):
    cut, want, count = cube_cut
    got, n = bm.host_label_volume(cut)
    assert n == count and np.array_equal(got, want)


@pytest.mark.parametrize("name", model.SHAPES)
def test_host_routine_equals_the_model_on_the_hand_made_shapes(bm, name):
    vol = model.shape(name)
    want, count, _ = model.model_labels(vol)
    assert count == model.SHAPE_COUNTS[name]
    got, n = bm.host_label_volume(vol)
    assert n == count and np.array_equal(got, want)
    # any non-zero byte is solid, and bool volumes are taken as they are
    assert np.array_equal(bm.host_label_volume(vol * np.uint8(200))[0], want) and np.array_equal(bm.host_label_volume(vol.astype(bool))[0], want)


def test_labels_are_one_plus_the_first_index_and_faces_alone_join():
    vol = np.zeros((3, 3, 3), np.uint8)
    vol[0, 0, 0] = vol[1, 1, 0] = vol[1, 1, 1] = vol[2, 2, 2] = 1   # (0,0,0) and (0,1,1) touch along an edge, (1,1,1) and (2,2,2) at a corner
    labels, count, _ = model.model_labels(vol)
    assert count == 3
    assert labels[0, 0, 0] == 1 and labels[1, 1, 0] == labels[1, 1, 1] == 1 + (1 * 3 + 1) * 3 + 0 and labels[2, 2, 2] == 27
    assert np.count_nonzero(labels) == 4


def test_scipy_gives_the_same_partition(bm, cube_cut):
    ndimage = pytest.importorskip("scipy.ndimage")
    cut, want, count = cube_cut
    for vol, labels, n in [(cut, want, count)] + [(model.shape(s),) + bm.host_label_volume(model.shape(s)) for s in model.SHAPES]:
        theirs, m = ndimage.label(vol)
        assert m == n and model.same_partition(theirs, labels)


def test_records_pin_the_tables_definition(cube_cut):
    """count, bounds, faces and ascending order, from the model's labels; the faces are those of the box clipped to the world"""
    cut, labels, count = cube_cut
    lo = (-5, 3, 0)     # the volume placed so that its first 5 columns lie outside a world of 64 x 51 x 40: the clipped box is x 0 ... 64, y 3 ... 51, z 0 ... 40
    world = (64, 51, 40)
    inside = np.zeros_like(labels)
    inside[:40, :48, 5:69] = labels[:40, :48, 5:69]   # (what a label volume holds: nothing outside the world)
    recs = model.model_records(inside, lo, world)
    assert (np.diff(recs["label"]) > 0).all() and recs["voxels"].sum() == np.count_nonzero(inside) and len(recs) == len(np.unique(inside)) - 1
    for r in recs[:: max(1, len(recs) // 40)]:
        zs, ys, xs = np.nonzero(inside == r["label"])
        xs, ys, zs = xs + lo[0], ys + lo[1], zs + lo[2]
        assert r["voxels"] == len(xs)
        assert tuple(r["lo"]) == (xs.min(), ys.min(), zs.min()) and tuple(r["hi"]) == (xs.max() + 1, ys.max() + 1, zs.max() + 1)
        faces = sum(1 << b for b, hit in enumerate([xs.min() == 0, xs.max() == 63, ys.min() == 3, ys.max() == 50, zs.min() == 0, zs.max() == 39]) if hit)
        assert r["faces"] == faces
    assert (recs["faces"] & 1).any() and (recs["faces"] & 2).any() and (recs["faces"] & 32).any() and (recs["faces"] == 0).any()
    assert model.COMPONENT_DTYPE.itemsize == 40


def test_python_door_refuses_wrong_volumes(bm):
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((2, 2, 2), np.int32), np.zeros((2, 2, 2), np.float32)):
        with pytest.raises(ValueError):
            bm.host_label_volume(bad)
    labels, n = bm.host_label_volume(np.zeros((0, 4, 4), np.uint8))
    assert n == 0 and labels.shape == (0, 4, 4)
    labels, n = bm.host_label_volume(np.ones((5, 6, 7), np.uint8)[::2, ::3, ::2])   # a strided view is copied
    assert n == 1 and (labels == 1).all()
    assert bm.COMPONENT_DTYPE == model.COMPONENT_DTYPE


# ---- the stand-alone program: the host routine linked alone, run plain and under the sanitizers
SRCS = [os.path.join(ROOT, "tests", "label_check.cpp"), os.path.join(ROOT, "brickmap_amd", "csrc", "label_host.cpp")]


def _run(exe, volumes):
    r = subprocess.run([str(exe), str(volumes)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "failures 0" in r.stdout, r.stdout + r.stderr
    words = r.stdout.split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def test_label_check_program(tmp_path):
    exe = tmp_path / "label_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe)] + SRCS)
    n = _run(exe, 40)
    assert n["volumes"] == 40 and n["voxels"] > 50_000 and n["components"] > 1_000 and n["bricks"] == 41 and n["refused"] == 6
    assert 20 <= n["rounds_max"] <= 512, "the snake through a brick takes dozens of rounds, and every brick settles within the bound"


def test_label_check_program_under_sanitizers(tmp_path):
    exe = tmp_path / "label_check_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe)] + SRCS)
    n = _run(exe, 12)
    assert n["volumes"] == 12 and n["bricks"] == 13 and n["refused"] == 6
