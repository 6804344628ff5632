"""Host half of bm_scene_load_voxels (CPU only): bm_host_load_supercell against a numpy model of the canonical build, the round trip
with the terrain generator, and the Python wrapper's argument checks."""
import numpy as np
import pytest

from _load_model import canonical_supercell, expand_supercell


def check_supercell(bm, volume, sx, sy, sz):
    words, bricks = bm.host_load_supercell(volume, sx, sy, sz)
    want_words, want_bricks = canonical_supercell(volume, sx, sy, sz)
    assert np.array_equal(words, want_words)
    assert np.array_equal(bricks, want_bricks)
    return words, bricks


@pytest.mark.parametrize("density", [0.0005, 0.02, 0.5, 0.97])
def test_random_volumes_match_the_model(bm, density):
    rng = np.random.default_rng(int(density * 10000))
    # any non-zero byte is solid: values from the whole range, in a world of 2 x 2 x 1 supercells with a different size along z
    volume = np.where(rng.random((128, 256, 256)) < density, rng.integers(1, 256, (128, 256, 256)), 0).astype(np.uint8)
    for sx, sy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        check_supercell(bm, volume, sx, sy, 0)


def test_bool_volume_and_tall_world(bm):
    rng = np.random.default_rng(7)
    volume = rng.random((384, 128, 128)) < 0.03
    for sz in range(3):
        check_supercell(bm, volume, 0, 0, sz)


def test_all_solid_supercell_has_4096_bricks(bm):
    volume = np.zeros((128, 256, 256), np.uint8)
    volume[:, 128:, :128] = 255  # supercell (0, 1, 0)
    words, bricks = check_supercell(bm, volume, 0, 1, 0)
    assert len(bricks) == 4096 and (bricks == 0xFFFFFFFF).all()
    assert words[4095] == (4095 | 0x80000000 | (0xFF << 12)) and np.array_equal(words & 0xFFF, np.arange(4096))
    for sx, sy in ((0, 0), (1, 0), (1, 1)):  # its neighbours are empty
        words, bricks = check_supercell(bm, volume, sx, sy, 0)
        assert not words.any() and len(bricks) == 0


def test_single_voxels_at_the_corners_of_a_supercell(bm):
    for corner in range(8):
        volume = np.zeros((256, 256, 256), np.uint8)
        x, y, z = 128 + 127 * (corner & 1), 128 + 127 * ((corner >> 1) & 1), 128 + 127 * (corner >> 2)
        volume[z, y, x] = 1
        words, bricks = check_supercell(bm, volume, 1, 1, 1)
        cell = 15 * (corner & 1) + 16 * 15 * ((corner >> 1) & 1) + 256 * 15 * (corner >> 2)
        assert np.count_nonzero(words) == 1 and words[cell] == (0x80000000 | (1 << corner) << 12) and len(bricks) == 1
        bit = 7 * (corner & 1) + 8 * 7 * ((corner >> 1) & 1) + 64 * 7 * (corner >> 2)
        assert bricks[0, bit >> 5] == 1 << (bit & 31) and np.count_nonzero(bricks) == 1
        for sc in range(7):  # nothing leaks into the other supercells
            assert not bm.host_load_supercell(volume, sc & 1, (sc >> 1) & 1, sc >> 2)[0].any()


def test_round_trip_with_the_generator(bm):
    G = 256
    volume = np.zeros((G, G, G), np.uint8)
    generated = {}
    for sc in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 1, 1), (0, 0, 1)):
        generated[sc] = bm.host_generate_supercell(G, G, *sc)
        expand_supercell(volume, *sc, *generated[sc])
    assert len(generated[(0, 0, 0)][1]) > 0
    for sc, (words, bricks) in generated.items():
        got_words, got_bricks = bm.host_load_supercell(volume, *sc)
        assert np.array_equal(got_words, words)
        assert np.array_equal(got_bricks, bricks)


def test_host_load_supercell_refuses_bad_arguments(bm):
    volume = np.zeros((128, 128, 128), np.uint8)
    with pytest.raises(bm.BrickmapError):
        bm.host_load_supercell(volume, 1, 0, 0)
    with pytest.raises(bm.BrickmapError):
        bm.host_load_supercell(volume, 0, 0, -1)


def test_volume_checks_raise_value_error(bm):
    import torch
    good = np.zeros((128, 256, 256), np.uint8)
    assert bm.volume_dims(good) == (256, 128)
    assert bm.volume_dims(good.view(np.bool_)) == (256, 128)
    assert bm.volume_dims(torch.zeros((256, 128, 128), dtype=torch.bool)) == (128, 256)
    assert bm.volume_dims(good, 256, 128) == (256, 128)
    bad = [
        np.zeros((128, 256, 128), np.uint8),              # not square in x and y
        np.zeros((128, 128), np.uint8),                   # not a volume
        np.zeros((100, 128, 128), np.uint8),              # not a multiple of 128
        np.zeros((0, 128, 128), np.uint8),
        np.zeros((128, 128, 128), np.int32),              # wrong dtype
        np.zeros((128, 128, 128), np.float32),
        np.zeros((128, 128, 256), np.uint8)[:, :, ::2],   # not contiguous
        np.zeros((128, 128, 128), np.uint8).transpose(2, 1, 0),
        torch.zeros((128, 128, 128), dtype=torch.float32),
        torch.zeros((128, 128, 256), dtype=torch.uint8)[:, :, ::2],
        [[[0]]],
    ]
    for volume in bad:
        with pytest.raises(ValueError):
            bm.volume_dims(volume)
        with pytest.raises(ValueError):  # ... and before a scene is made of it (no GPU is touched)
            bm.Scene.from_voxels(volume)
    with pytest.raises(ValueError):
        bm.volume_dims(good, 128, 128)  # a right volume for another scene
    with pytest.raises(ValueError):
        bm.host_load_supercell(np.zeros((128, 128, 128), np.int16), 0, 0, 0)
