"""Shared cases of the connected-component tests, and a restatement of the labelling that is written differently from the product's
host form (which cuts rows into runs and joins them by a union-find): a plain flood fill over a padded copy, position by position.

The shapes are the smallest at which each path of csrc/ptb_components.hip can go wrong.  Its tiles are T = 16 x 64 positions (2-D) and
4 x 8 x 32 (3-D), its chunks 1024 consecutive positions: T - 1, T, T + 1 and 2 T + 1 in each direction, 1 x 1, 1 x N, N x 1, widths
that are no multiple of 4 (peeled loads), a view at an odd base offset, and one 1030 x 1027 spiral and serpentine whose chains cross
hundreds of workgroups.  Every pattern has its seed fixed."""
import functools

import numpy as np

TILE_2D = (16, 64)
TILE_3D = (4, 8, 32)


# ---------------------------------------------------------------------------------------------------------------- patterns
def _rng(seed):
    return np.random.default_rng(seed)


def zeros(shape):
    return np.zeros(shape, np.uint8)


def ones(shape):
    return np.ones(shape, np.uint8)


def checkerboard(shape):
    return (np.indices(shape).sum(0) % 2).astype(np.uint8)


def noise(shape, seed, classes=2):
    return _rng(seed).integers(0, classes, shape).astype(np.uint8)


def speckle(shape, seed):
    return (_rng(seed).random(shape) < 0.03).astype(np.uint8)


def blobs(shape, seed, classes=6, cell=5):
    """labels6-style: a coarse random class map blown up into blocky multi-class blobs"""
    coarse = _rng(seed).integers(0, classes, [(s + cell - 1) // cell for s in shape]).astype(np.uint8)
    for axis in range(len(shape)):
        coarse = np.repeat(coarse, cell, axis=axis)
    return np.ascontiguousarray(coarse[tuple(slice(0, s) for s in shape)])


def serpentine(H, W):
    """one component that winds through every other row; the connectors alternate between the last and the first column"""
    a = np.zeros((H, W), np.uint8)
    a[0::2] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        a[y, W - 1 if k % 2 == 0 else 0] = 1
    return a


def serpentine_3d(D, H, W):
    """the 2-D serpentine on every other slice; single voxels join the slices alternately at its end and at its start"""
    s = serpentine(H, W)
    last = H - 1 if H % 2 else H - 2                          # the serpentine's last row
    turns = len(range(1, H - 1, 2))
    end = (last, W - 1 if turns % 2 == 0 else 0)
    a = np.zeros((D, H, W), np.uint8)
    a[0::2] = s
    for k, z in enumerate(range(1, D - 1, 2)):
        y, x = end if k % 2 == 0 else (0, 0)
        a[z, y, x] = 1
    return a


def spiral(H, W):
    """a square spiral, one position wide with one position between its turns"""
    a = np.zeros((H, W), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    a[0, 0] = 1
    while True:
        for _ in range(2):
            ny, nx, ny2, nx2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < H and 0 <= nx < W and not a[ny, nx] and not (0 <= ny2 < H and 0 <= nx2 < W and a[ny2, nx2]):
                y, x = ny, nx
                a[y, x] = 1
                break
            dy, dx = dx, -dy
        else:
            return a


def diagonals(H, W):
    """two diagonal staircases that touch only by corners: separate under 4, one component under 8"""
    a = np.zeros((H, W), np.uint8)
    for r in range(H):
        for c in (r, r + 1, r - 3, r - 2):
            if 0 <= c < W:
                a[r, c] = 1
    return a


def touching(H, W):
    """blobs of different classes that touch: they must not merge"""
    a = np.ones((H, W), np.uint8)
    a[:, W // 2:] = 2
    a[H // 4:H // 2, W // 4:3 * W // 4] = 3
    a[-2:, :] = 0
    return a


# name -> (array, dims); "offset" cases are handed to the device as a view one element into a larger buffer
def _cases():
    (ty, tx), (vz, vy, vx) = TILE_2D, TILE_3D
    c = {}
    c["one"] = (ones((1, 1)), 2)
    c["row"] = (noise((1, 2 * tx + 3), 1), 2)
    c["column"] = (noise((2 * ty + 1, 1), 2), 2)
    c["zeros"] = (zeros((ty + 1, tx + 1)), 2)
    c["ones"] = (ones((2 * ty + 1, 2 * tx + 1)), 2)
    c["ones_wide"] = (ones((2 * ty, 2 * tx)), 2)
    c["checkerboard"] = (checkerboard((ty + 1, tx + 1)), 2)
    c["checkerboard_T"] = (checkerboard((ty, tx)), 2)
    c["blobs"] = (blobs((2 * ty + 1, 2 * tx + 1), 3), 2)
    c["blobs_wide"] = (blobs((2 * ty, 2 * tx), 4), 2)
    c["noise_T-1"] = (noise((ty - 1, tx - 1), 5), 2)
    c["noise_T"] = (noise((ty, tx), 6), 2)
    c["noise_T+1"] = (noise((ty + 1, tx + 1), 7), 2)
    c["noise_2T+1"] = (noise((2 * ty + 1, 2 * tx + 1), 8), 2)
    c["noise4_wide"] = (noise((3 * ty, 2 * tx + 4), 9, classes=4), 2)
    c["noise_W%4"] = (noise((ty + 3, tx + 2), 10), 2)
    c["noise_offset"] = (noise((2 * ty, 2 * tx), 11), 2)
    c["speckle"] = (speckle((2 * ty + 1, 2 * tx + 2), 12), 2)
    c["serpentine"] = (serpentine(2 * ty + 1, 2 * tx + 1), 2)
    c["spiral"] = (spiral(2 * ty + 1, 2 * tx + 1), 2)
    c["diagonals"] = (diagonals(2 * ty + 8, tx + 6), 2)
    c["touching"] = (touching(ty + 4, tx + 6), 2)
    c["stack"] = (np.stack([noise((37, 53), 13), blobs((37, 53), 14), serpentine(37, 53)]), 2)
    c["spiral_big"] = (spiral(1030, 1027), 2)
    c["serpentine_big"] = (serpentine(1030, 1027), 2)
    c["volume_noise"] = (noise((9, 17, 23), 15), 3)
    c["volume_blobs"] = (blobs((33, 34, 35), 16, classes=4, cell=6), 3)
    c["volume_serpentine"] = (serpentine_3d(2 * vz + 1, 2 * vy + 1, vx + 1), 3)
    c["volume_ones"] = (ones((vz + 1, vy + 1, vx + 1)), 3)
    c["volume_checkerboard"] = (checkerboard((vz + 1, vy + 1, vx + 1)), 3)
    c["volume_noise_T-1"] = (noise((vz - 1, vy - 1, vx - 1), 17), 3)
    c["volume_noise_T"] = (noise((vz, vy, vx), 18), 3)
    c["volume_noise_2T+1"] = (noise((2 * vz + 1, 2 * vy + 1, 2 * vx + 1), 19, classes=3), 3)
    c["volume_noise_wide"] = (noise((2 * vz, 2 * vy, 2 * vx), 20), 3)
    c["volume_offset"] = (noise((vz + 1, vy, vx), 21), 3)
    c["volume_stack"] = (noise((2, 2, 9, 17, 23), 22, classes=3), 3)
    return c


CASES = _cases()
OFFSET_CASES = ("noise_offset", "volume_offset")
BIG_CASES = ("spiral_big", "serpentine_big")
CONNECTIVITIES = {2: (4, 8), 3: (6, 26)}


# ---------------------------------------------------------------------------------------------------------------- restatement
def _offsets(dims, connectivity):
    full = connectivity in (8, 26)
    out = []
    for d in np.ndindex(*(3,) * dims):
        d = tuple(int(v) - 1 for v in d)
        if any(d) and (full or sum(abs(v) for v in d) == 1):
            out.append(d)
    return out


def _fill_entry(a, connectivity, background):
    """flood fill of one entry: (cc, n, areas, boxes, values)"""
    dims = a.ndim
    padded = np.zeros([s + 2 for s in a.shape], dtype=np.int64)            # (the border becomes None below: it equals no value)
    inner = tuple(slice(1, -1) for _ in range(dims))
    padded[inner] = a
    vals = padded.reshape(-1).tolist()
    if background is not None:
        vals = [None if v == background else v for v in vals]
    pad_mask = np.ones(padded.shape, dtype=bool)
    pad_mask[inner] = False
    for i in np.flatnonzero(pad_mask.reshape(-1)).tolist():
        vals[i] = None
    strides = [int(np.prod(padded.shape[k + 1:])) for k in range(dims)]
    offs = [sum(o * s for o, s in zip(d, strides)) for d in _offsets(dims, connectivity)]
    lab = [0] * len(vals)
    n = 0
    order = np.flatnonzero(~pad_mask.reshape(-1)).tolist()                 # row-major over the entry
    for s in order:
        v = vals[s]
        if v is None or lab[s]:
            continue
        n += 1
        lab[s] = n
        todo = [s]
        while todo:
            p = todo.pop()
            for o in offs:
                q = p + o
                if lab[q] == 0 and vals[q] == v:
                    lab[q] = n
                    todo.append(q)
    cc = np.array(lab, dtype=np.int32).reshape(padded.shape)[inner]
    areas = np.bincount(cc.reshape(-1), minlength=n + 1)[1:].astype(np.int64)
    boxes = np.zeros((n, 2 * dims), np.int64)
    values = np.zeros(n, a.dtype)
    coords = np.nonzero(cc)
    ids = cc[coords]
    for k in range(n):
        sel = ids == k + 1
        for d in range(dims):
            boxes[k, d] = coords[d][sel].min()
            boxes[k, dims + d] = coords[d][sel].max() + 1
        values[k] = a[tuple(cd[sel][0] for cd in coords)]
    return np.ascontiguousarray(cc), n, areas, boxes, values


def restate(a, dims, connectivity, background=0):
    """The labelling of ``a`` ([*stack, (D,) H, W]) by flood fill: a dict with ``cc`` (int32 like a), ``count`` (int64, stack-shaped) and
    per entry (lists in stack order) ``areas``, ``boxes``, ``values``."""
    a = np.asarray(a)
    stack = a.shape[:a.ndim - dims]
    entries = a.reshape((-1,) + a.shape[a.ndim - dims:])
    res = [_fill_entry(e, connectivity, background) for e in entries]
    return {"cc": np.stack([r[0] for r in res]).reshape(a.shape) if len(res) else np.zeros(a.shape, np.int32),
            "count": np.array([r[1] for r in res], np.int64).reshape(stack),
            "areas": [r[2] for r in res], "boxes": [r[3] for r in res], "values": [r[4] for r in res]}


@functools.lru_cache(maxsize=None)
def expected(name, connectivity, as_bool=False, background=0):
    """restate() of a case, computed once per session and shared; as_bool: of the map ``case != 0`` (what a bool tensor holds)"""
    a, dims = CASES[name]
    if as_bool:
        a = (a != 0)
    return restate(a, dims, connectivity, background)


def remove_small(a, dims, connectivity, min_area, background=0, fill=None, ref=None):
    """what remove_small_components returns, from the flood fill"""
    ref = ref or restate(a, dims, connectivity, background)
    fill = background if fill is None else fill
    out = np.array(a, copy=True)
    entries = out.reshape((-1,) + out.shape[out.ndim - dims:])
    ccs = ref["cc"].reshape(entries.shape)
    for e, cc, areas in zip(entries, ccs, ref["areas"]):
        small = np.concatenate([[False], areas < min_area])[cc]
        e[small] = fill
    return out
