"""The temporal accumulation of bm_reproject / bm_host_reproject as a numpy float32 model, written from the specification
(include/brickmap.h), not from csrc/reproject.h -- and the synthetic cases the host and GPU tests share.

Every array is float32 and every operation one IEEE operation on float32 operands, in the order the specification gives, so the model's
result is the library's bit for bit.  A skipped tap is an np.where that keeps the running sum (nothing is multiplied by zero)."""
import collections
import functools

import numpy as np

from _denoise_model import HIT_DTYPE, SPECIAL, keys

F = np.float32
Cam = collections.namedtuple("Cam", "position direction up")


def _v(x):
    return [F(c) for c in x]


def _cross(x, y):
    return [x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1]]


def _normalize(v):
    inv = F(1) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return [c * inv for c in v]


def _sq(v):
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def basis(cam, w, h):
    """the frames' view basis for a w x h image: origin, dir, right = normalize(cross(dir, up)) * 1.5 * aspect, up = normalize(cross(right, dir)) * 1.5"""
    with np.errstate(all="ignore"):
        d, upv = _v(cam.direction), _v(cam.up)
        aspect = F(w) / F(h)
        right = [(c * F(1.5)) * aspect for c in _normalize(_cross(d, upv))]
        up = [c * F(1.5) for c in _normalize(_cross(right, d))]
    return _v(cam.position), d, right, up


def pixel_dirs(cam, w, h):
    """three float32 [h, w] arrays: the direction of the centre ray of every pixel, as bm_camera_pixel_rays gives it for (x + 0.5, y + 0.5)"""
    _, d, right, up = basis(cam, w, h)
    W, H = F(w), F(h)
    px = (np.arange(w, dtype=F) + F(0.5))[None, :].repeat(h, axis=0)
    py = (np.arange(h, dtype=F) + F(0.5))[:, None].repeat(w, axis=1)
    with np.errstate(all="ignore"):
        ppx, ppy = px - F(1), py - F(1)
        ni = (ppx / W) - F(0.5)
        nj = ((H - ppy) / H) - F(0.5)
        v = [(d[k] + right[k] * ni) + up[k] * nj for k in range(3)]
        inv = F(1) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        return [(c * inv).astype(F) for c in v]


def reproject(cur, prev, accum, hits, prev_image, prev_keys, max_history=32.0):
    """accum: float32 [H, W, 4] and hits: HIT_DTYPE [H * W] of camera `cur`; prev_image float32 [H, W, 4] and prev_keys uint32 [H, W] of
    camera `prev`, or None, None -> (image float32 [H, W, 4], keys uint32 [H, W])"""
    accum = np.asarray(accum, F)
    h, w = accum.shape[:2]
    key = keys(accum, hits)
    out = accum.copy()
    if prev_image is None:
        return out, key
    prev_image, prev_keys = np.asarray(prev_image, F).reshape(h, w, 4), np.asarray(prev_keys, np.uint32).reshape(h, w)
    W, H, mh = F(w), F(h), F(max_history)
    o, _, _, _ = basis(cur, w, h)
    o2, D2, R2, U2 = basis(prev, w, h)
    dhat = pixel_dirs(cur, w, h)
    dist = hits["distance"].reshape(h, w).astype(F)
    with np.errstate(all="ignore"):
        dd, rr, uu = _sq(D2), _sq(R2), _sq(U2)
        e = [(o[k] + dhat[k] * dist) - o2[k] for k in range(3)]
        t = ((e[0] * D2[0] + e[1] * D2[1]) + e[2] * D2[2]) / dd
        ok = (key != SPECIAL) & (t > 0)
        a = ((e[0] * R2[0] + e[1] * R2[1]) + e[2] * R2[2]) / (t * rr)
        b = ((e[0] * U2[0] + e[1] * U2[1]) + e[2] * U2[2]) / (t * uu)
        u = (a + F(0.5)) * W + F(0.5)
        v = (H - (b + F(0.5)) * H) + F(0.5)
        x0f, y0f = np.floor(u), np.floor(v)
        fx, fy = u - x0f, v - y0f
        ok &= (x0f >= F(-1)) & (x0f <= W - F(1)) & (y0f >= F(-1)) & (y0f <= H - F(1))
        x0 = np.where(ok, x0f, F(0)).astype(np.int64)
        y0 = np.where(ok, y0f, F(0)).astype(np.int64)
        gx, gy = F(1) - fx, F(1) - fy
        taps = [(0, 0, gx * gy), (1, 0, fx * gy), (0, 1, gx * fy), (1, 1, fx * fy)]
        Ws, N = np.zeros((h, w), F), np.zeros((h, w), F)
        C = [np.zeros((h, w), F) for _ in range(3)]
        counted = np.zeros((h, w), bool)
        for dx, dy, wgt in taps:
            qx, qy = x0 + dx, y0 + dy
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            kq, vq = prev_keys[cy, cx], prev_image[cy, cx]
            nq = vq[..., 3]
            cnt = ok & inside & (kq == key) & (nq > 0) & (wgt > 0)
            Ws = np.where(cnt, Ws + wgt, Ws)
            C = [np.where(cnt, C[k] + wgt * (vq[..., k] / nq), C[k]) for k in range(3)]
            N = np.where(cnt, N + wgt * nq, N)
            counted |= cnt
        n_h = N / Ws
        n_h = np.where(n_h < mh, n_h, mh)
        for k in range(3):
            out[..., k] = np.where(counted, (C[k] / Ws) * n_h + accum[..., k], accum[..., k])
        out[..., 3] = np.where(counted, n_h + accum[..., 3], accum[..., 3])
    return out.astype(F), key


# ---- the synthetic world: a floor slab and two towers, integer boxes [lo, hi); a camera's hit records come from a slab test.  They need
# only be consistent with themselves: distance, entry normal, voxel, level 2 -- and misses above the horizon
BOXES = [((0, 0, 0), (512, 512, 4)), ((240, 238, 4), (248, 246, 20)), ((258, 244, 4), (264, 254, 30))]


def cast(cam, w, h):
    """HIT_DTYPE [h * w]: the first hit of every pixel's centre ray of `cam` in the world of BOXES (cameras stand outside every box)"""
    d = np.stack(pixel_dirs(cam, w, h), axis=-1).astype(np.float64).reshape(-1, 3)
    o = np.asarray(cam.position, F).astype(np.float64)
    n = len(d)
    hits = np.zeros(n, HIT_DTYPE)
    hits["distance"] = np.inf
    hits["voxel"] = -1
    hits["level"] = -1
    best = np.full(n, np.inf)
    with np.errstate(all="ignore"):
        for lo, hi in BOXES:
            lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
            t1, t2 = (lo - o) / d, (hi - o) / d
            tn, tf = np.minimum(t1, t2), np.maximum(t1, t2)
            axis = np.argmax(tn, axis=-1)
            tnear, tfar = tn.max(axis=-1), tf.min(axis=-1)
            hit = np.isfinite(d).all(axis=-1) & (tnear < tfar) & (tnear > 0) & (tnear < best)
            idx = np.nonzero(hit)[0]
            ax = axis[idx]
            p = o + d[idx] * tnear[idx, None]
            vox = np.clip(np.floor(p), lo, hi - 1).astype(np.int32)
            from_low = d[idx, ax] > 0  # the ray travels up the axis: it enters through the low face
            vox[np.arange(len(idx)), ax] = np.where(from_low, lo[ax], hi[ax] - 1).astype(np.int32)
            nrm = np.zeros((len(idx), 3), F)
            nrm[np.arange(len(idx)), ax] = np.where(from_low, -1, 1)
            hits["distance"][idx] = tnear[idx].astype(F)
            hits["normal"][idx] = nrm
            hits["voxel"][idx] = vox
            hits["level"][idx] = 2
            best[idx] = tnear[idx]
    return hits


def look(position, direction, up=(0.0, 0.0, 1.0)):
    d = _normalize(_v(direction))
    return Cam(tuple(float(F(c)) for c in position), tuple(float(c) for c in d), tuple(float(c) for c in up))


def _moved(cam, delta):
    return cam._replace(position=tuple(float(F(F(p) + F(s))) for p, s in zip(cam.position, delta)))


def camera_pairs():
    """(name, current camera, previous camera)"""
    cur = look((250.0, 200.0, 34.0), (0.08, 0.8, -0.5))
    d = np.asarray(cur.direction, np.float64)
    side = np.cross(d, (0, 0, 1))
    side /= np.linalg.norm(side)
    yaw = 0.05
    turned = (d[0] * np.cos(yaw) - d[1] * np.sin(yaw), d[0] * np.sin(yaw) + d[1] * np.cos(yaw), d[2])
    return [
        ("identical", cur, cur),
        ("sideways", cur, _moved(cur, 0.5 * side)),           # half a voxel
        ("forward", cur, _moved(cur, -1.5 * d)),              # the camera advanced: the previous one stood behind
        ("yaw", cur, look(cur.position, turned)),
        ("turned_round", cur, look(cur.position, -d)),        # everything lies behind the previous camera
        ("far_jump", cur, _moved(cur, 4000.0 * side)),        # every reprojection leaves the image
        ("from_above", cur, Cam((251.5, 242.25, 90.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))),  # straight down, up = +y
        ("degenerate", cur, Cam((251.5, 242.25, 90.0), (0.0, 0.0, -1.0), (0.0, 0.0, 1.0))),  # dir parallel to up: NaNs, so no history
    ]


SIZES = [(33, 17), (64, 64), (257, 65)]  # width x height: pixel counts that 256 does not divide, or several workgroups of one row


def _noisy(rng, h, w, n):
    rgb = rng.exponential(0.6, (h, w, 3)).astype(F) * n[..., None]
    return np.concatenate([rgb, n[..., None]], axis=-1).astype(F)


Case = collections.namedtuple("Case", "name cur prev accum hits prev_image prev_keys")


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for si, (w, h) in enumerate(SIZES):
        for pi, (name, cur, prev) in enumerate(camera_pairs()):
            rng = np.random.default_rng(1000 + 10 * si + pi)
            # the frame just rendered: 1 spp, some pixels without a terminated path
            n = (rng.integers(0, 12, (h, w)) > 0).astype(F)
            accum = _noisy(rng, h, w, n)
            hits = cast(cur, w, h)
            # the history: sample counts 0 ... 48, whole and fractional, some above max_history, some zero
            pn = np.where(rng.integers(0, 10, (h, w)) == 0, 0, rng.uniform(0.25, 48.0, (h, w))).astype(F)
            whole = rng.integers(0, 2, (h, w)) == 0
            pn = np.where(whole, np.ceil(pn), pn).astype(F)
            prev_image = _noisy(rng, h, w, pn)
            prev_keys = keys(np.where(pn[..., None] > 0, prev_image, F(1)), cast(prev, w, h))  # (a pixel without samples still has its surface)
            out.append(Case(f"{name}_{w}x{h}", cur, prev, accum, hits, prev_image, prev_keys))
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name, max_history=32.0):
    c = case(name)
    return reproject(c.cur, c.prev, c.accum, c.hits, c.prev_image, c.prev_keys, max_history)


def history(image, key):
    """the buffer of a history: the image's words, then the keys, as float32 words"""
    return np.concatenate([np.ascontiguousarray(image, F).reshape(-1), np.ascontiguousarray(key, np.uint32).reshape(-1).view(F)])
