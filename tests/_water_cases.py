"""The volumes the water tests share (tests/test_water_host.py on the CPU, tests/test_gpu_water.py on the device): each case is
(name, volume [z, y, x] uint8, drains or None, open faces, sea_level).  Built once; nobody writes to them."""
import numpy as np

SIDES = ("-x", "+x", "-y", "+y")


def block(shape, top):
    """solid below z = top, free from there up"""
    vol = np.zeros(shape, np.uint8)
    vol[:top] = 1
    return vol


def bowl(shape=(8, 12, 12), top=5, lo=2, a=4, b=8):
    vol = block(shape, top)
    vol[lo:top, a:b, a:b] = 0
    return vol


def u_tube(nx=12, left=2, right=8):
    """two shafts joined at the bottom; the right one stands in a tower three voxels higher: both arms fill to the left rim"""
    vol = block((14, 5, nx), 10)
    vol[10:13, 1:4, right - 1:right + 2] = 7
    vol[1:10, 2, left] = 0
    vol[1:13, 2, right] = 0
    vol[1, 2, left:right + 1] = 0
    return vol


def pit_with_tunnel():
    """the bowl's pit, and a tunnel from its floor to the -x side: it drains"""
    vol = bowl()
    vol[2, 5, :4] = 0
    return vol


def air_bell():
    """a chamber that rises above its only entrance: everything in it runs off downwards"""
    vol = np.ones((10, 7, 9), np.uint8)
    vol[1, 3, :5] = 0      # the entrance tunnel from the -x side
    vol[1:8, 2:5, 4:7] = 0  # the chamber above and beside it
    return vol


def closed_cave():
    vol = bowl()
    vol[0:2, 1:3, 1:4] = 0
    vol[0, 9, 9] = 0
    return vol


def serpentine(nx=24, ny=16):
    """a corridor at z = 1 that runs along x, turns at the far end, runs back ...: one end on the -x side, every other voxel solid"""
    vol = np.ones((3, ny, nx), np.uint8)
    rows = list(range(1, ny - 1, 2))
    for k, y in enumerate(rows):
        vol[1, y, 1:nx - 1] = 0
        if k + 1 < len(rows):
            vol[1, y + 1, nx - 2 if k % 2 == 0 else 1] = 0
    vol[1, rows[0], 0] = 0
    return vol


def late_detour():
    """a shaft at the far end is reached first along a high corridor (bottleneck 10), later along a low zigzag that crosses a tile face
    every other step (bottleneck 1): its values fall twice"""
    vol = np.ones((12, 16, 40), np.uint8)
    vol[10, 3, :39] = 0                 # the high corridor from the -x side
    vol[1:11, 3, 38] = 0                # the shaft
    y = 7
    for x in range(0, 38, 2):           # the low zigzag at z = 1 between y = 7 and y = 8, the face of two tiles
        vol[1, 7:9, x] = 0
        vol[1, y, x:x + 3] = 0
        y = 15 - y
    vol[1, 3:9, 38] = 0                 # its end joins the shaft's foot
    return vol


def random_volume(seed, density, shape=(19, 20, 24)):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def _cases():
    out = [("one free", np.zeros((1, 1, 1), np.uint8), None, SIDES, 0), ("one solid", np.ones((1, 1, 1), np.uint8), None, SIDES, 0),
           ("bowl", bowl(), None, SIDES, 0), ("u-tube", u_tube(), None, SIDES, 0), ("pit with tunnel", pit_with_tunnel(), None, SIDES, 0),
           ("air bell", air_bell(), None, SIDES, 0), ("closed cave", closed_cave(), None, SIDES, 0),
           ("drained bowl", bowl(), [(5, 5, 2)], SIDES, 0),
           ("rejected drains", bowl(), [(-1, 0, 0), (12, 0, 0), (0, 12, 0), (0, 0, 8), (0, 0, 0), (5, 5, 2), (5, 5, 2)], SIDES, 0)]
    for face in ("-x", "+x", "-y", "+y", "-z", "+z"):
        out.append((f"open {face}", random_volume(7, 0.45, (9, 10, 11)), None, (face,), 0))
    out.append(("no open face", random_volume(7, 0.45, (9, 10, 11)), None, (), 0))
    out.append(("no open face, a drain", bowl(), [(5, 5, 3)], (), 0))
    for sea in (0, 4, 8):
        out.append((f"sea {sea}", bowl(), None, SIDES, sea))
    out.append(("sea 3, random", random_volume(8, 0.5, (9, 10, 11)), None, SIDES + ("+z",), 3))
    return out


CASES = _cases()
RANDOM = [(f"random {density} seed {seed}", random_volume(seed, density), None, SIDES, 0) for density in (0.5, 0.6, 0.7) for seed in (0, 1, 2)]
