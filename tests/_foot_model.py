"""A numpy model of ground navigation, written from the contract in include/brickmap.h alone (the comment above bm_foot_params): the room
bytes by a downward loop over every column, the field by a plain queue search over legal moves, a path by the rule as a loop.  Slow and
obvious.  And the named cases that tests/test_foot_host.py and tests/test_gpu_foot.py share: the smallest shapes at which each rule can
go wrong."""
import collections

import numpy as np

NONE = 0x7FFFFFFF
RESULT_DTYPE = np.dtype([("reached", "<u8"), ("farthest", "<u4"), ("seeds_rejected", "<u4"), ("farthest_at", "<u8"), ("standable", "<u8")])
COLUMNS = ((-1, 0), (1, 0), (0, -1), (0, 1))   # -x, +x, -y, +y

Case = collections.namedtuple("Case", "volume floor seeds height climb drop toward max_steps")


def case(volume, seeds, height=2, climb=1, drop=3, toward=False, max_steps=0, floor=True):
    return Case(volume, floor, [tuple(int(v) for v in s) for s in seeds], height, climb, drop, toward, max_steps)


# ---------------------------------------------------------------- the model
def model_room(volume, floor=True):
    nz, ny, nx = volume.shape
    room = np.zeros((nz, ny, nx), np.uint8)
    for y in range(ny):
        for x in range(nx):
            free = 127   # everything above the volume is free
            for z in range(nz - 1, -1, -1):
                if volume[z, y, x]:
                    free = 0
                    continue
                free = min(free + 1, 127)
                below = bool(volume[z - 1, y, x]) if z > 0 else floor
                room[z, y, x] = free | (0x80 if below else 0)
    return room


def lists(room):
    """the room bytes as nested lists [z][y][x] of ints: what stand and legal read (an array is converted on every call, so callers in a
    loop convert once)"""
    return room if isinstance(room, list) else np.asarray(room).tolist()


def stand(room, p, height):
    v = lists(room)[p[2]][p[1]][p[0]]
    return bool(v & 0x80) and (v & 0x7F) >= height


def legal(room, p, q, height, climb, drop):
    """is p -> q a legal move of the agent"""
    room = lists(room)
    nz, ny, nx = len(room), len(room[0]), len(room[0][0])
    if (q[0] - p[0], q[1] - p[1]) not in COLUMNS or not (0 <= q[0] < nx and 0 <= q[1] < ny and 0 <= q[2] < nz):
        return False
    dz = q[2] - p[2]
    if not (stand(room, p, height) and stand(room, q, height) and -drop <= dz <= climb):
        return False
    lower = p if dz >= 0 else q
    return (room[lower[2]][lower[1]][lower[0]] & 0x7F) >= height + abs(dz)


def moves_from(room, p, height, climb, drop):
    """the targets of the legal moves from p, the columns in the order -x, +x, -y, +y and inside a column in ascending z"""
    for dx, dy in COLUMNS:
        for dz in range(-drop, climb + 1):
            q = (p[0] + dx, p[1] + dy, p[2] + dz)
            if legal(room, p, q, height, climb, drop):
                yield q


def model_field(room, seeds, height=2, climb=1, drop=3, toward=False, max_steps=0):
    nz, ny, nx = room.shape
    room_array, room = room, lists(room)
    if toward:   # the moves from p to a seed: the same search with climb and drop exchanged
        climb, drop = drop, climb
    field = np.full((nz, ny, nx), NONE, np.uint32)
    queue, rejected = collections.deque(), 0
    for x, y, z in seeds:
        if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz) or not stand(room, (x, y, z), height):
            rejected += 1
        elif field[z, y, x] == NONE:
            field[z, y, x] = 0
            queue.append((x, y, z))
    while queue:
        p = queue.popleft()
        level = int(field[p[2], p[1], p[0]]) + 1
        if max_steps and level > max_steps:
            continue
        for q in moves_from(room, p, height, climb, drop):
            if field[q[2], q[1], q[0]] == NONE:
                field[q[2], q[1], q[0]] = level
                queue.append(q)
    finite = field != NONE
    rec = np.zeros((), RESULT_DTYPE)
    rec["reached"], rec["seeds_rejected"] = int(finite.sum()), rejected
    rec["standable"] = len(stands_of(room_array, height))
    rec["farthest"] = int(field[finite].max()) if finite.any() else NONE
    rec["farthest_at"] = int(np.argmax(field.ravel() == rec["farthest"])) if finite.any() else 0
    return field.view(np.int32), rec


def model_paths(room, field, starts, capacity, height=2, climb=1, drop=3, toward=False):
    nz, ny, nx = room.shape
    room = lists(room)
    field = np.asarray(field).view(np.uint32)
    path = np.full((len(starts), capacity, 3), -1, np.int32)
    lengths = np.zeros(len(starts), np.int32)
    for i, (x, y, z) in enumerate(starts):
        if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz) or field[z, y, x] == NONE:
            continue
        p, t = (int(x), int(y), int(z)), int(field[z, y, x])
        lengths[i] = t + 1
        path[i, 0] = p
        for k in range(1, min(t + 1, capacity)):
            nxt = None
            for dx, dy in COLUMNS:
                qx, qy = p[0] + dx, p[1] + dy
                if not (0 <= qx < nx and 0 <= qy < ny):
                    continue
                for qz in range(nz):
                    q = (qx, qy, qz)
                    if field[qz, qy, qx] == t - 1 and (legal(room, p, q, height, climb, drop) if toward else legal(room, q, p, height, climb, drop)):
                        nxt = q
                        break
                if nxt:
                    break
            if nxt is None:
                lengths[i] = -1
                break
            p, t = nxt, t - 1
            path[i, k] = p
    return path, lengths


def stands_of(room, height):
    """the stands in linear order, as (x, y, z)"""
    z, y, x = np.nonzero(((room & 0x80) != 0) & ((room & 0x7F) >= height))
    return list(zip(x.tolist(), y.tolist(), z.tolist()))


def voxel_of(index, shape):
    nz, ny, nx = shape
    return (int(index) % nx, int(index) // nx % ny, int(index) // (nx * ny))


# ---------------------------------------------------------------- the named cases
def terrace(tops, nz, ny=1):
    """a row of columns along x, column x blocked up to and including z = tops[x] (-1: not at all)"""
    v = np.zeros((nz, ny, len(tops)), np.uint8)
    for x, top in enumerate(tops):
        v[: top + 1, :, x] = 1
    return v


def serpentine():
    v = np.ones((2, 24, 24), np.uint8)
    v[1, 0::2, :] = 0
    for i, y in enumerate(range(1, 24, 2)):
        v[1, y, 23 if i % 2 == 0 else 0] = 0
    return v


RANDOM_SHAPE = (23, 29, 37)
RANDOM_AGENTS = ((1, 1, 3), (2, 1, 3), (2, 2, 8))
RANDOM = [(s, density, agent, toward) for s in range(6) for density in (0.2, 0.3) for agent in RANDOM_AGENTS for toward in (False, True)]


def random_name(s, density, agent, toward):
    return f"random {s} at {density}, agent {agent[0]}-{agent[1]}-{agent[2]}" + (", toward" if toward else "")


def random_case(s, density, agent, toward):
    volume = (np.random.default_rng(s).random(RANDOM_SHAPE) < density).astype(np.uint8)
    stands = stands_of(model_room_fast(volume), agent[0])
    return case(volume, stands[:: len(stands) // 8][:8], *agent, toward=toward)


def model_room_fast(volume, floor=True):
    """model_room by whole slices (the same downward loop, vectorised over the columns); test_foot_host.py holds the two together"""
    nz = volume.shape[0]
    room = np.zeros(volume.shape, np.uint8)
    free = np.full(volume.shape[1:], 127, np.int64)
    for z in range(nz - 1, -1, -1):
        free = np.where(volume[z] != 0, 0, np.minimum(free + 1, 127))
        below = (volume[z - 1] != 0) if z > 0 else np.full(volume.shape[1:], floor)
        room[z] = free | np.where((free != 0) & below, 0x80, 0)
    return room


NAMES = ["one voxel", "one voxel, no floor", "room saturates", "step of one, step of two: climb 1", "step of one, step of two: climb 2",
         "ledge of three: seeded on top", "ledge of three: seeded at the bottom", "ledge of three: toward", "ledge of three: drop 2 from the top",
         "ledge of three: drop 2 from the bottom", "lintel: height 1", "lintel: height 2", "head bump", "two storeys", "wide front", "serpentine",
         "serpentine, cut in the middle", "pitched", "seeds", "no seeds"] + [random_name(*r) for r in RANDOM]

_cases = {}


def cases():
    if _cases:
        return _cases
    c = _cases
    c["one voxel"] = case(np.zeros((1, 1, 1), np.uint8), [(0, 0, 0)])
    c["one voxel, no floor"] = case(np.zeros((1, 1, 1), np.uint8), [(0, 0, 0)], floor=False)
    # column (0, 0) open to the sky above a blocked voxel, column (1, 0) the same under a ceiling at z = 139, the rest solid
    v = np.ones((140, 2, 3), np.uint8)
    v[1:, 0, 0] = 0
    v[1:139, 0, 1] = 0
    c["room saturates"] = case(v, [(0, 0, 1)])
    steps = terrace([0, 0, 1, 1, 3, 3], 8)
    c["step of one, step of two: climb 1"] = case(steps, [(0, 0, 1)], climb=1)
    c["step of one, step of two: climb 2"] = case(steps, [(0, 0, 1)], climb=2)
    ledge = terrace([3, 3, 3, 0, 0, 0], 8)
    c["ledge of three: seeded on top"] = case(ledge, [(0, 0, 4)], drop=3)
    c["ledge of three: seeded at the bottom"] = case(ledge, [(5, 0, 1)], drop=3)
    c["ledge of three: toward"] = case(ledge, [(5, 0, 1)], drop=3, toward=True)
    c["ledge of three: drop 2 from the top"] = case(ledge, [(0, 0, 4)], drop=2)
    c["ledge of three: drop 2 from the bottom"] = case(ledge, [(5, 0, 1)], drop=2, toward=True)
    lintel = terrace([0] * 7, 5)
    lintel[2, 0, 3] = 1   # the ceiling at head height: one free voxel under it
    c["lintel: height 1"] = case(lintel, [(0, 0, 1)], height=1)
    c["lintel: height 2"] = case(lintel, [(0, 0, 1)], height=2)
    bump = terrace([0, 0, 1, 1], 8)
    bump[3, 0, 1] = 1     # the lower voxel (1, 0, 1) has R = 2 = h: no room to rise by one
    c["head bump"] = case(bump, [(0, 0, 1)], height=2, climb=1)
    storeys = terrace([0, 0, 0], 6)
    storeys[2, 0, 1] = 1  # column 1 holds stands at z = 1 (R = 1) and z = 3
    c["two storeys"] = case(storeys, [(0, 0, 1)], height=1, climb=2, drop=3)
    plain = np.zeros((2, 96, 96), np.uint8)
    plain[0] = 1
    c["wide front"] = case(plain, [(48, 48, 1)])
    c["serpentine"] = case(serpentine(), [(0, 0, 1)], climb=0)
    c["serpentine, cut in the middle"] = case(serpentine(), [(0, 0, 1)], climb=0, max_steps=150)
    big = (np.random.default_rng(7).random((20, 24, 40)) < 0.2).astype(np.uint8)
    c["pitched"] = case(big[2:17, 3:20, 5:30], [(3, 3, 0), (20, 10, 0), (12, 8, 5)])   # a view: row and slice pitch above the extents
    v = terrace([0] * 6, 6, ny=3)
    v[2, 1, 4] = 1        # (4, 1, 1) lies under a low ceiling; (4, 1, 3) stands on it
    c["seeds"] = case(v, [(-1, 0, 1), (6, 0, 1), (0, 3, 1), (0, 0, 6), (2, 1, 0), (2, 1, 3), (4, 1, 1), (1, 1, 1), (1, 1, 1), (4, 1, 3), (1, 1, 1)])
    c["no seeds"] = case(v, [])
    for r in RANDOM:
        c[random_name(*r)] = random_case(*r)
    return c
