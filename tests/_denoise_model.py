"""The a-trous filter of bm_denoise / bm_host_denoise as a numpy float32 model, written from the specification (include/brickmap.h,
DESIGN.md 4.12), not from csrc/denoise.h -- and the synthetic cases the host and GPU tests share.

Every array is float32 and every operation one IEEE operation on float32 operands, in the order the specification gives, so the model's
result is the library's bit for bit.  A skipped tap is an np.where that keeps the running sum (nothing is multiplied by zero)."""
import functools

import numpy as np

F = np.float32
SPECIAL = np.uint32(0xFFFFFFFF)
HIT_DTYPE = np.dtype([("distance", "<f4"), ("normal", "<f4", 3), ("voxel", "<i4", 3), ("level", "<i4")])  # bm_ray_hit
H5 = (F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16))


def radiance(accum):
    n = accum[..., 3]
    ok = n > 0
    with np.errstate(all="ignore"):
        return [np.where(ok, accum[..., k] / n, F(0)).astype(F) for k in range(3)]


def luminance(c):
    return (F(0.2126) * c[0] + F(0.7152) * c[1]) + F(0.0722) * c[2]


def keys(accum, hits):
    """uint32 [H, W]: plane * 8 + axis * 2 + side, SPECIAL for pixels that are not filtered"""
    h, w = accum.shape[:2]
    hits = hits.reshape(h, w)
    nrm, vox, lvl = hits["normal"], hits["voxel"].astype(np.int64), hits["level"]
    nonzero = nrm != 0
    special = ~(accum[..., 3] > 0) | (lvl < 0) | (lvl > 2) | ~nonzero.any(axis=-1)
    a = np.argmax(nonzero, axis=-1)  # the first axis whose normal component is not zero
    na = np.take_along_axis(nrm, a[..., None], axis=-1)[..., 0]
    s = (na > 0).astype(np.int64)
    size = np.where(lvl == 2, 1, np.where(lvl == 1, 4, 8))
    plane = np.take_along_axis(vox, a[..., None], axis=-1)[..., 0] + s * size
    key = (plane * 8 + a * 2 + s) & 0xFFFFFFFF
    return np.where(special, SPECIAL, key.astype(np.uint32)).astype(np.uint32)


def _shift(img, dx, dy, fill):
    """out[y, x] = img[y + dy, x + dx], `fill` outside the image"""
    h, w = img.shape
    out = np.full_like(img, fill)
    ys, ye = max(0, -dy), min(h, h - dy)
    xs, xe = max(0, -dx), min(w, w - dx)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = img[ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def denoise(accum, hits, iterations=5, sigma_l=4.0):
    """accum: float32 [H, W, 4]; hits: HIT_DTYPE [H * W] -> float32 [H, W, 4] = (c, 1)"""
    accum = np.asarray(accum, F)
    h, w = accum.shape[:2]
    key = keys(accum, hits)
    filtered = key != SPECIAL
    c = radiance(accum)
    sigma = F(sigma_l)
    with np.errstate(all="ignore"):
        if iterations > 0:
            # variance pass: 7 x 7 at stride 1
            lum = luminance(c)
            tot = [np.zeros((h, w), F) for _ in range(3)]
            for dy in range(-3, 4):
                row = [np.zeros((h, w), F) for _ in range(3)]
                for dx in range(-3, 4):
                    ok = filtered & (_shift(key, dx, dy, SPECIAL) == key)
                    lq = _shift(lum, dx, dy, F(0))
                    row[0] = np.where(ok, row[0] + F(1), row[0])
                    row[1] = np.where(ok, row[1] + lq, row[1])
                    row[2] = np.where(ok, row[2] + lq * lq, row[2])
                tot = [t + r for t, r in zip(tot, row)]
            n = np.where(filtered, tot[0], F(1))
            mean = tot[1] / n
            v = tot[2] / n - mean * mean
            var = np.where(v > 0, v, F(0)).astype(F)
        for i in range(iterations):
            step = 1 << i
            lum = luminance(c)
            den = sigma * np.sqrt(var) + F(1e-4)
            tot = [np.zeros((h, w), F) for _ in range(5)]  # W, C.r, C.g, C.b, V
            for ky in range(5):
                row = [np.zeros((h, w), F) for _ in range(5)]
                for kx in range(5):
                    dx, dy = (kx - 2) * step, (ky - 2) * step
                    ok = filtered & (_shift(key, dx, dy, SPECIAL) == key)
                    x = np.abs(lum - _shift(lum, dx, dy, F(0))) / den
                    t = F(1) + x
                    wgt = (H5[ky] * H5[kx]) / (t * t)
                    terms = [wgt] + [wgt * _shift(c[k], dx, dy, F(0)) for k in range(3)] + [(wgt * wgt) * _shift(var, dx, dy, F(0))]
                    row = [np.where(ok, r + term, r) for r, term in zip(row, terms)]
                tot = [t_ + r for t_, r in zip(tot, row)]
            wsum = np.where(filtered, tot[0], F(1))
            c = [np.where(filtered, tot[1 + k] / wsum, c[k]).astype(F) for k in range(3)]
            var = np.where(filtered, tot[4] / (wsum * wsum), var).astype(F)
    return np.stack(c + [np.ones((h, w), F)], axis=-1).astype(F)


# ---- synthetic cases: (name, accum [H, W, 4], hits [H * W])
def make_hits(h, w):
    hits = np.zeros(h * w, HIT_DTYPE)
    hits["distance"] = 10
    hits["normal"][:, 2] = 1
    hits["voxel"][:] = (5, 6, 7)
    hits["level"] = 2
    return hits


def _noisy(rng, h, w):
    """exponential, 1-spp-like radiance: (R, G, B, n) with n = 1 ... 3 terminated paths"""
    n = rng.integers(1, 4, (h, w)).astype(F)
    rgb = rng.exponential(0.6, (h, w, 3)).astype(F) * n[..., None]
    return np.concatenate([rgb, n[..., None]], axis=-1).astype(F)


def _set(hits, idx, normal, voxel, level):
    hits["normal"][idx] = normal
    hits["voxel"][idx] = voxel
    hits["level"][idx] = level


NORMALS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def scene_case(seed, h, w):
    """the general case: vertical bands of the six normal directions, a plane shared by the three LoD levels, misses, unresolved bricks,
    zero normals, pixels without samples, one-pixel-wide surfaces, a lone pixel, a constant region"""
    rng = np.random.default_rng(seed)
    accum = _noisy(rng, h, w)
    hits = make_hits(h, w).reshape(h, w)
    for x in range(w):
        nrm = NORMALS[(x * 6) // max(w, 1) % 6]
        _set(hits, (slice(None), x), nrm, (40, 48, 56), 2)
    # levels 0, 1, 2 whose entry faces share the plane z = 64 seen from above (normal +z: plane = voxel + size), row by row
    for y in range(h):
        lvl = y % 3
        size = (8, 4, 1)[lvl]
        hits["normal"][y, : w // 3] = (0, 0, 1)
        hits["voxel"][y, : w // 3] = (8 * (y % 5), 16, 64 - size)
        hits["level"][y, : w // 3] = lvl
    # a surface one pixel wide (a column and a row), when there is room
    if w >= 9:
        _set(hits, (slice(None), w // 2), (0, -1, 0), (3, 77, 3), 2)
    if h >= 9:
        _set(hits, (h // 2, slice(None)), (-1, 0, 0), (91, 3, 3), 1)
    # special pixels scattered about: a miss, an unresolved brick, a zero normal, no samples
    kinds = rng.integers(0, 12, (h, w))
    hits["level"][kinds == 0] = -1
    hits["voxel"][kinds == 0] = -1
    hits["normal"][kinds == 0] = 0
    hits["level"][kinds == 1] = 3
    hits["normal"][kinds == 2] = 0
    accum[kinds == 3] = 0  # n = 0
    # a constant region (var = 0) in the lower right quarter of the +z band
    accum[h // 2:, (2 * w) // 3:] = (F(0.5), F(0.25), F(0.125), F(1))
    # a pixel whose key is alone in the whole image
    _set(hits, (h - 1, w - 1), (0, 0, -1), (1000, 1000, 1000), 2)
    accum[h - 1, w - 1] = (F(3), F(2), F(1), F(2))
    return accum, hits.reshape(-1)


SIZES = [(1, 1), (9, 1), (1, 9), (37, 70), (3, 129)]  # (height, width): 1x1, 1x9, 9x1, 70x37, 129x3 as width x height


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for k, (h, w) in enumerate(SIZES):
        accum, hits = scene_case(100 + k, h, w)
        out.append((f"scene_{w}x{h}", accum, hits))
    # a constant image on one surface: var = 0 everywhere
    h, w = 12, 17
    out.append(("constant_17x12", np.tile(np.array([0.75, 0.5, 0.25, 1], F), (h, w, 1)), make_hits(h, w)))
    # noisy radiance on one surface, and split by a vertical key boundary
    rng = np.random.default_rng(7)
    out.append(("noisy_40x33", _noisy(rng, 33, 40), make_hits(33, 40)))
    hits = make_hits(33, 40).reshape(33, 40)
    _set(hits, (slice(None), slice(20, 40)), (1, 0, 0), (9, 9, 9), 2)
    out.append(("two_planes_40x33", _noisy(rng, 33, 40), hits.reshape(-1)))
    return out


@functools.lru_cache(maxsize=None)
def expected(name, iterations, sigma_l=4.0):
    _, accum, hits = next(c for c in cases() if c[0] == name)
    return denoise(accum, hits, iterations, sigma_l)
