"""Shared cases of the watershed tests, and an evaluation of the definition of utils/watershed.py that is written differently from the
product's host form (ONE flood over ``(pass height, steps, seed)`` on a padded grid) and from the kernels (tile sweeps): TWO shortest-path
searches with bounds-checked neighbours -- first the pass height ``C`` alone (a minimax Dijkstra), then, with ``C`` final, the fewest
admissible steps and the smallest seed (a Dijkstra over ``(steps, seed)`` that only takes steps ``q -> p`` with ``C(q) <= C(p)``).  Also the
brute-force UNAMBIGUOUS check: one pass-height map per marker label; where exactly one label attains ``C(p)``, every flooding watershed
must give that label.

Every case stays near 20 k positions so that the model takes about a second at most; expectations are computed once per session."""
import functools
import heapq

import numpy as np
from scipy import ndimage

import nearest_cases as NC

CONNECTIVITIES = {2: (4, 8), 3: (6, 26)}


# ---------------------------------------------------------------------------------------------------------------- the model
def _neighbours(shape, full):
    dims = len(shape)
    offs = [o for o in np.ndindex(*(3,) * dims) if any(v != 1 for v in o) and (full or sum(abs(v - 1) for v in o) == 1)]
    offs = [tuple(v - 1 for v in o) for o in offs]
    strides = [int(np.prod(shape[k + 1:])) for k in range(dims)]

    def around(p):
        c, r = [], p
        for s in strides:
            c.append(r // s)
            r %= s
        for o in offs:
            if all(0 <= c[k] + o[k] < shape[k] for k in range(dims)):
                yield p + sum(o[k] * strides[k] for k in range(dims))

    return around


def pass_height(h, in_m, seeds, full):
    """``C`` of one entry as a flat float64 array (``inf``: no path): ``h`` heights, ``in_m`` the flooded set, ``seeds`` flat indices"""
    around = _neighbours(h.shape, full)
    hl, ok = h.ravel().tolist(), in_m.ravel().tolist()
    cost = [float("inf")] * len(hl)
    done = [False] * len(hl)
    heap = [(hl[s], s) for s in seeds if ok[s]]
    heapq.heapify(heap)
    while heap:
        c, p = heapq.heappop(heap)
        if done[p]:
            continue
        done[p], cost[p] = True, c
        for n in around(p):
            if ok[n] and not done[n]:
                heapq.heappush(heap, (max(c, hl[n]), n))
    return np.array(cost)


def flood_entry(h, in_m, seed_mask, full):
    """``(C, sigma)`` of one entry, flat: float64 with ``inf``, int64 with -1"""
    seeds = np.flatnonzero(seed_mask.ravel() & in_m.ravel()).tolist()
    cost = pass_height(h, in_m, seeds, full)
    around = _neighbours(h.shape, full)
    cl = cost.tolist()
    sigma = [-1] * len(cl)
    heap = [(0, s, s) for s in seeds]
    heapq.heapify(heap)
    while heap:
        d, s, p = heapq.heappop(heap)
        if sigma[p] >= 0:
            continue
        sigma[p] = s
        for n in around(p):
            if sigma[n] < 0 and cl[n] != float("inf") and cl[p] <= cl[n]:
                heapq.heappush(heap, (d + 1, s, n))
    return cost, np.array(sigma, np.int64)


def _wrap(background, dtype):
    dtype = np.dtype(dtype)
    if dtype == np.bool_:
        return background in (0, 1), bool(background)
    info = np.iinfo(dtype)
    return info.min <= background <= info.max, (background - info.min) % (info.max - info.min + 1) + info.min


class Case:
    """``height`` (float32 / float16 / uint8 / int16 array), ``markers`` (integer array), ``mask`` (bool array or None) of one shape ``[*stack, <dims axes>]``"""

    def __init__(self, name, height, markers, mask=None, dims=2, background=0):
        assert height.shape == markers.shape and (mask is None or mask.shape == markers.shape)
        self.name, self.height, self.markers, self.mask, self.dims, self.background = name, height, markers, mask, dims, background

    def __repr__(self):
        return self.name

    def entries(self, a):
        return a.reshape((-1,) + a.shape[a.ndim - self.dims:])

    @functools.cached_property
    def flooded(self):
        h = self.height.astype(np.float64)
        ok = ~np.isnan(h) & (h != np.inf)
        return ok if self.mask is None else ok & (self.mask != 0)

    @functools.cached_property
    def seeds(self):
        fits, _ = _wrap(self.background, self.markers.dtype)
        return self.flooded & ((self.markers != self.background) if fits else True)

    @functools.lru_cache(maxsize=None)
    def expected(self, connectivity):
        """``(labels, cost float32, seed int32)`` of the definition; -0.0 counts as +0.0, also in the cost"""
        full = connectivity == CONNECTIVITIES[self.dims][1]
        h = np.where(self.flooded, self.height.astype(np.float64), 0.0) + 0.0
        labels = np.empty_like(self.markers)
        cost = np.empty(self.markers.shape, np.float32)
        seed = np.empty(self.markers.shape, np.int32)
        fill = self.markers.dtype.type(_wrap(self.background, self.markers.dtype)[1])
        for he, me, se, ke, le, ce, ie in zip(*(self.entries(a) for a in (h, self.flooded, self.seeds, self.markers, labels, cost, seed))):
            c, s = flood_entry(he, me, se, full)
            ce[...] = c.reshape(ce.shape)
            ie[...] = s.reshape(ie.shape)
            le[...] = np.where(s >= 0, ke.ravel()[np.maximum(s, 0)], fill).reshape(le.shape)
        for a in (labels, cost, seed):
            a.setflags(write=False)
        return labels, cost, seed

    def unambiguous(self, connectivity):
        """``(where, label)``: the positions at which exactly one marker label attains the pass height, and that label"""
        full = connectivity == CONNECTIVITIES[self.dims][1]
        h = np.where(self.flooded, self.height.astype(np.float64), 0.0) + 0.0
        where = np.zeros(self.markers.shape, bool)
        label = np.zeros(self.markers.shape, np.int64)
        for he, me, se, ke, we, le in zip(*(self.entries(a) for a in (h, self.flooded, self.seeds, self.markers, where, label))):
            values = np.unique(ke[se])
            per = np.stack([pass_height(he, me, np.flatnonzero((se & (ke == v)).ravel()).tolist(), full) for v in values]) if len(values) else np.zeros((0, he.size))
            if not len(values):
                continue
            best = per.min(axis=0)
            attains = (per == best) & np.isfinite(best)
            we[...] = (attains.sum(axis=0) == 1).reshape(we.shape)
            le[...] = values[attains.argmax(axis=0)].reshape(le.shape)
        return where, label


def bfs_expected(markers, in_m, full):
    """a constant landscape: multi-source breadth-first search, a position taking the smallest seed index among its predecessors' of the
    level before -- ``(labels, seed)`` of a 2-D map with background 0"""
    shape = markers.shape
    around = _neighbours(shape, full)
    ok = in_m.ravel().tolist()
    sigma = np.full(markers.size, -1, np.int64)
    level = [p for p in np.flatnonzero((markers != 0).ravel()).tolist() if ok[p]]
    for p in level:
        sigma[p] = p
    while level:
        offered = {}
        for p in level:
            for n in around(p):
                if ok[n] and sigma[n] < 0:
                    offered[n] = min(offered.get(n, sigma[p]), sigma[p])
        for n, s in offered.items():
            sigma[n] = s
        level = list(offered)
    labels = np.where(sigma >= 0, markers.ravel()[np.maximum(sigma, 0)], 0).astype(markers.dtype)
    return labels.reshape(shape), sigma.reshape(shape).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- generators
def blob_map(shape, seed, count=9, radius=(9, 17)):
    """a semantic map of overlapping discs (balls in 3-D)"""
    rng = np.random.default_rng(seed)
    grid = np.indices(shape)
    sem = np.zeros(shape, bool)
    for _ in range(count):
        c = [rng.integers(0, s) for s in shape]
        r = rng.integers(*radius)
        sem |= sum((g - v) ** 2 for g, v in zip(grid, c)) <= r * r
    return sem


def edt_case(name, shape, seed, core, **kw):
    sem = blob_map(shape, seed, **kw)
    d = ndimage.distance_transform_edt(sem).astype(np.float32)
    cores, n = ndimage.label(d > core, structure=np.ones((3,) * len(shape)))
    assert n >= 4, (name, n)
    return Case(name, -d, cores.astype(np.int32), sem, len(shape))


def smooth_noise(shape, seed, sigma=3.0):
    return ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), sigma).astype(np.float32)


def point_seeds(shape, seed, count, dtype=np.int32):
    rng = np.random.default_rng(seed)
    m = np.zeros(int(np.prod(shape)), dtype)
    m[rng.choice(m.size, count, replace=False)] = np.arange(1, count + 1)
    return m.reshape(shape)


def serpentine(rows, cols, horizontal=True):
    """a corridor one position wide that runs along every other row and turns at alternating ends; one seed at its start"""
    mask = np.zeros((rows, cols), bool)
    mask[::2] = True
    for k, r in enumerate(range(1, rows, 2)):
        mask[r, cols - 1 if k % 2 == 0 else 0] = True
    markers = np.zeros((rows, cols), np.int32)
    markers[0, 0] = 5
    return (mask, markers) if horizontal else (np.ascontiguousarray(mask.T), np.ascontiguousarray(markers.T))


def _cases():
    c = {}

    def add(case):
        assert case.name not in c
        c[case.name] = case

    add(edt_case("blobs_edt", (96, 120), 11, 3.0))                                                  # the real workload shape
    sem, _ = NC.two_discs()
    d = ndimage.distance_transform_edt(sem).astype(np.float32)
    add(Case("two_discs", -d, ndimage.label(d > 8, structure=np.ones((3, 3)))[0].astype(np.int32), sem != 0))
    add(Case("smooth_points", smooth_noise((100, 131), 12), point_seeds((100, 131), 13, 12)))       # long winding optimal paths
    rng = np.random.default_rng(14)
    add(Case("u8_noise_holes", rng.integers(0, 6, (90, 110)).astype(np.uint8), point_seeds((90, 110), 15, 25, np.uint8), rng.random((90, 110)) >= 0.1))       # masses of ties
    add(Case("constant", np.full((70, 90), 2.5, np.float32), point_seeds((70, 90), 16, 9), rng.random((70, 90)) >= 0.15))
    for horizontal in (True, False):                                                                # about 2000 steps inside a tile, across the tile edges
        mask, markers = serpentine(66, 66, horizontal)
        add(Case(f"serpentine_{'h' if horizontal else 'v'}", np.zeros((66, 66), np.float32), markers, mask))
    mask, markers = serpentine(130, 131)                                                            # more sweeps than a batch launches
    add(Case("serpentine_long", np.linspace(0, 1, 130 * 131, dtype=np.float32).reshape(130, 131), markers, mask))
    for e in (63, 64, 65, 66, 129):                                                                 # one position either side of a tile edge, and a third tile
        add(Case(f"rows{e}", smooth_noise((e, 70), 20 + e), point_seeds((e, 70), 30 + e, 5)))
        add(Case(f"cols{e}", smooth_noise((70, e), 40 + e), point_seeds((70, e), 50 + e, 5)))
    add(Case("odd_width", smooth_noise((37, 53), 60), point_seeds((37, 53), 61, 6), rng.random((37, 53)) >= 0.1))      # total % 4 != 0: peeled loads
    h = smooth_noise((3, 40, 44), 62)
    m = point_seeds((3, 40, 44), 63, 9)
    m[1] = 0
    add(Case("stack_hole", h, m))                                                                   # an entry without seeds
    mask = rng.random((50, 60)) >= 0.3
    m = point_seeds((50, 60), 64, 40)
    assert ((m != 0) & ~mask).any() and ((m != 0) & mask).any()
    add(Case("seeds_outside_mask", smooth_noise((50, 60), 65), m, mask))
    h = smooth_noise((50, 60), 66)
    h[rng.random((50, 60)) < 0.08] = np.nan
    h[rng.random((50, 60)) < 0.08] = np.inf
    h[rng.random((50, 60)) < 0.05] = -np.inf
    m = point_seeds((50, 60), 67, 30)
    assert np.isnan(h[m != 0]).any() or np.isinf(h[m != 0]).any()
    add(Case("nan_inf", h, m))
    h = np.where(rng.random((40, 48)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)  # -0.0 against +0.0: one plateau
    h[rng.random((40, 48)) < 0.1] = 1.0
    assert np.signbit(h).any()
    add(Case("signed_zero", h, point_seeds((40, 48), 68, 5)))
    add(Case("background_unheld", smooth_noise((20, 24), 69), point_seeds((20, 24), 70, 7, np.uint8), rng.random((20, 24)) >= 0.2, background=300))
    add(Case("background_7", smooth_noise((30, 36), 71), np.where(rng.random((30, 36)) < 0.03, rng.integers(0, 3, (30, 36)), 7).astype(np.int16), background=7))
    # 3-D: bricks are 8 x 8 x 32
    add(Case("volume", smooth_noise((10, 19, 70), 72, 2.0), point_seeds((10, 19, 70), 73, 10), rng.random((10, 19, 70)) >= 0.05, dims=3))
    add(edt_case("volume_edt", (17, 24, 40), 74, 3.0, count=10, radius=(4, 7)))
    corridor = np.zeros((9, 17, 33), bool)                                                           # a 3-D corridor: serpentines in every other slice, joined at alternating corners
    for z in range(0, 9, 2):
        corridor[z] = serpentine(17, 33)[0]
    for k, z in enumerate(range(1, 9, 2)):
        corridor[(z, 16, 32) if k % 2 == 0 else (z, 0, 0)] = True
    m = np.zeros((9, 17, 33), np.int32)
    m[0, 0, 0] = 3
    add(Case("volume_corridor", np.zeros((9, 17, 33), np.float32), m, corridor, dims=3))
    m = point_seeds((3, 9, 10, 35), 75, 12)
    m[2] = 0
    add(Case("volume_stack", smooth_noise((3, 9, 10, 35), 76, 1.5), m, dims=3))
    for shape in ((8, 8, 32), (7, 9, 31), (9, 7, 33), (17, 9, 65)):                                  # either side of a brick edge, and a third brick
        add(Case("brick%dx%dx%d" % shape, smooth_noise(shape, 77 + shape[0] + shape[2], 1.5), point_seeds(shape, 78 + shape[1], 4), dims=3))
    return c


CASES = _cases()
assert all(c.markers.size <= 21_000 for c in CASES.values()), [n for n, c in CASES.items() if c.markers.size > 21_000]
PAIRS = [(n, k) for n, c in CASES.items() for k in CONNECTIVITIES[c.dims]]
UNAMBIGUOUS_CASES = ("blobs_edt", "two_discs", "volume_edt")
