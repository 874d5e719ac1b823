"""Shared cases of the nearest-site and label-expansion tests, and restatements that are written differently from the product's host form
(which takes minima shift by shift, axis by axis, and carries the site along): all-pairs brute forces that take the FIRST minimum over
``np.argwhere(sites)`` -- row-major order makes the first minimum the smallest linear index, the tie rule of utils/nearest.py.

The cases are those of tests/distance_cases.py (zeros are the sites): its shapes are the ones at which the kernels of
csrc/ptb_nearest.hip can go wrong, since they walk rows and lines exactly as the distance kernels do.  The exact index is expected on
every case of at most BRUTE_LIMIT positions per entry; the others -- VALIDITY_ONLY, asserted below to be exactly four -- are checked by
validity (the returned site lies at scipy's distance) and against the host form.  scipy breaks ties differently: it is a yardstick for
validity only, never for the index."""
import functools

import numpy as np

import distance_cases as DC

CASES = DC.CASES
BRUTE_LIMIT = DC.BRUTE_LIMIT
EXACT_SPACINGS = ((2.0, 0.5, 1.0), (1.0, 4.0, 0.25))      # powers of two: every squared distance of the small cases is exact in float32


def entry_size(name):
    a, dims = CASES[name]
    return int(np.prod(a.shape[a.ndim - dims:]))


SMALL = tuple(n for n in CASES if entry_size(n) <= BRUTE_LIMIT)
VALIDITY_ONLY = tuple(n for n in CASES if n not in SMALL)
assert len(CASES) == 111 and sorted(VALIDITY_ONLY) == ["serpentine_big", "spiral_big", "volume_big", "wide_one_site"], VALIDITY_ONLY
EXACT_SPACING_CASES = tuple(n for n in DC.SPACING_CASES if n in SMALL)


# ---------------------------------------------------------------------------------------------------------------- restatement
def brute_nearest(sites, dims, weights=None):
    """``(squared distance, index)`` of every position of ``sites`` ([*stack, <dims axes>]) to the nearest True of its entry: the first minimum
    over the sites in row-major order; the index counts within the entry, -1 (and DC.INF / inf) without a site.  int64 squared index
    distances, or with ``weights`` (the squared spacings of the ``dims`` axes) float64."""
    sites = np.asarray(sites, dtype=bool)
    ent = sites.reshape((-1,) + sites.shape[sites.ndim - dims:])
    dist = np.full(ent.shape, DC.INF if weights is None else np.inf, np.int64 if weights is None else np.float64)
    index = np.full(ent.shape, -1, np.int64)
    for e, od, oi in zip(ent, dist, index):
        s = np.argwhere(e).astype(np.int64)
        if not len(s):
            continue
        lin = np.ravel_multi_index(tuple(s.T), e.shape)
        p = np.argwhere(np.ones(e.shape, bool)).astype(np.int64)
        step = max(1, 4_000_000 // len(s))
        bd, bi = od.reshape(-1), oi.reshape(-1)
        for k in range(0, len(p), step):
            d = np.zeros((len(p[k:k + step]), len(s)), dist.dtype)
            for axis in range(dims):
                off = p[k:k + step, axis, None] - s[None, :, axis]
                d += off * off if weights is None else weights[axis] * (off * off).astype(np.float64)
            first = d.argmin(axis=1)                                           # (numpy: the first of equal minima)
            bd[k:k + step] = d[np.arange(len(first)), first]
            bi[k:k + step] = lin[first]
    return dist.reshape(sites.shape), index.reshape(sites.shape)


@functools.lru_cache(maxsize=None)
def expected_index(name):
    """int64 index map of a small case, computed once per session and shared"""
    a, dims = CASES[name]
    assert name in SMALL
    dist, index = brute_nearest(a == 0, dims)
    assert np.array_equal(dist, DC.expected(name))
    index.setflags(write=False)
    return index


@functools.lru_cache(maxsize=None)
def expected_index_spacing(name, spacing):
    """the same under a spacing of EXACT_SPACINGS.  Asserts what makes the comparison exact: every value a pass of the kernels stores --
    the squared distance within the row, within the slice, within the volume -- is a float32."""
    a, dims = CASES[name]
    assert name in EXACT_SPACING_CASES and spacing in EXACT_SPACINGS
    w = tuple(s * s for s in spacing[-dims:])
    for axes in range(1, dims + 1):
        part, index = brute_nearest(a == 0, axes, w[dims - axes:])
        fin = np.isfinite(part)
        assert np.array_equal(part[fin].astype(np.float32).astype(np.float64), part[fin]), (name, spacing, axes)
    index.setflags(write=False)
    return index


def squared_to(index, shape, dims, spacing=None):
    """the squared distance from every position to the site ``index`` names (an int index map of ``shape``, >= 0 everywhere): exact int64, or
    float64 under ``spacing``"""
    ent = shape[len(shape) - dims:]
    here = np.indices(ent).reshape((dims,) + (1,) * (len(shape) - dims) + tuple(ent))
    there = np.stack(np.unravel_index(np.asarray(index, np.int64), ent))
    off = np.broadcast_to(here, there.shape) - there
    if spacing is None:
        return (off * off).sum(axis=0)
    w = np.asarray(spacing[-dims:], np.float64).reshape((dims,) + (1,) * len(shape))
    return ((off * w) ** 2).sum(axis=0)


def check_valid(index, name, what=""):
    """``index`` (int array) names, at every position of the case, a site at the exact minimum distance; -1 exactly in entries without one"""
    a, dims = CASES[name]
    index = np.asarray(index).astype(np.int64)
    want = DC.expected(name) if name in SMALL else DC.scipy_squared(a == 0, dims)
    none = want >= DC.INF
    assert np.array_equal(index < 0, none) and bool((index[none] == -1).all()), (name, what)
    ent = a.shape[a.ndim - dims:]
    assert bool((index < int(np.prod(ent))).all()), (name, what)
    sites = (a == 0).reshape((-1,) + (int(np.prod(ent)),))
    idx = np.maximum(index, 0).reshape(sites.shape)
    assert bool(np.take_along_axis(sites, idx, axis=1)[~none.reshape(sites.shape)].all()), (name, what, "not a site")
    assert np.array_equal(squared_to(np.maximum(index, 0), a.shape, dims)[~none], want[~none]), (name, what, "not a nearest site")


# ---------------------------------------------------------------------------------------------------------------- label expansion
class Expansion:
    def __init__(self, name, markers, dims=2, distance=None, mask=None, background=0, spacing=None, offset=False):
        self.name, self.markers, self.dims, self.distance, self.mask = name, markers, dims, distance, mask
        self.background, self.spacing, self.offset = background, spacing, offset

    def __repr__(self):
        return self.name

    @functools.cached_property
    def expected(self):
        out = restate_expansion(self.markers, self.dims, self.distance, self.mask, self.background, self.spacing)
        out.setflags(write=False)
        return out


def restate_expansion(markers, dims, distance, mask, background, spacing):
    """the definition, position by position: a labelled position keeps its value; another one takes the value at its nearest labelled
    position (first minimum in row-major order) if that is within ``distance`` and the mask is set there; else the background"""
    m = np.asarray(markers)
    weights = None if spacing is None else tuple(s * s for s in spacing)
    dist, index = brute_nearest(m != background, dims, weights)
    ent = m.reshape((-1, int(np.prod(m.shape[m.ndim - dims:]))))
    out = ent.copy()
    for e, o, d, i, k in zip(ent, out, dist.reshape(ent.shape), index.reshape(ent.shape), (np.ones(m.shape, bool) if mask is None else np.asarray(mask) != 0).reshape(ent.shape)):
        for p in range(len(e)):
            if e[p] != background:
                continue
            ok = i[p] >= 0 and k[p] and (distance is None or float(d[p]) <= float(distance) * float(distance))
            o[p] = e[i[p]] if ok else background
    return out.reshape(m.shape)


def sparse_markers(shape, seed, dtype=np.int32, p=0.02, ids=7):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < p, rng.integers(1, ids + 1, shape), 0).astype(dtype)


def random_mask(shape, seed, p=0.6):
    return np.random.default_rng(seed).random(shape) < p


EXPANSION_SHAPES = (((5, 257), 2), ((65, 6), 2), ((3, 21, 45), 2), ((2, 5, 9, 21), 3))
DISTANCES = (None, 0, 1, 2.5, 1e9)


def _expansions():
    c = []
    for k, (shape, dims) in enumerate(EXPANSION_SHAPES):                               # (a) the shapes x distance x mask
        m = sparse_markers(shape, 300 + k)
        for dist in DISTANCES:
            for masked in (False, True):
                c.append(Expansion(f"a{shape}-{dist}-{'mask' if masked else 'all'}", m, dims, dist, random_mask(shape, 320 + k) if masked else None))
    shape, dims = EXPANSION_SHAPES[2]
    base = sparse_markers(shape, 302)
    for dtype in (np.uint8, np.int16, np.int64, bool):                                  # (b) the other element types
        c.append(Expansion(f"b-{np.dtype(dtype).name}", base.astype(dtype), dims, 2.5, random_mask(shape, 322)))
        c.append(Expansion(f"b-{np.dtype(dtype).name}-unlimited", base.astype(dtype), dims))
    rng = np.random.default_rng(340)                                                    # (c) another background on a map that holds zeros
    other = np.where(rng.random((21, 45)) < 0.03, rng.choice([0, 0, 1, 2, 5], (21, 45)), 3).astype(np.int32)
    assert (other == 0).any()
    c.append(Expansion("c-background3", other, 2, 4.0, random_mask((21, 45), 341), background=3))
    c.append(Expansion("c-background-unheld", base.astype(np.uint8), dims, background=300))      # occurs nowhere: every position is labelled
    hole = base.copy()                                                                  # (d) an entry without a marker inside a stack
    hole[1] = 0
    c.append(Expansion("d-stack-hole", hole, dims))
    c.append(Expansion("d-stack-hole-masked", hole, dims, 6.0, random_mask(shape, 342)))
    c.append(Expansion("e-offset", sparse_markers((20, 64), 343), 2, 3.0, random_mask((20, 64), 344), offset=True))     # (e) a misaligned base
    c.append(Expansion("e-offset-int64", sparse_markers((5, 6, 128), 345, np.int64), 3, offset=True))
    c.append(Expansion("g-spacing", sparse_markers((21, 45), 346), 2, 3.0, spacing=(2.0, 0.5)))       # the float32 comparison of the gather
    c.append(Expansion("g-spacing3", sparse_markers((5, 9, 21), 347), 3, 2.0, random_mask((5, 9, 21), 348), spacing=(1.0, 4.0, 0.25)))
    return c


EXPANSIONS = _expansions()


# ---------------------------------------------------------------------------------------------------------------- the two-disc split
def two_discs():
    """``(sem, truth)``: two overlapping discs of radius 10 on a (40, 60) map -- one connected object -- and the instance map that gives every
    object pixel to the nearer centre, ties to the first disc"""
    y, x = np.mgrid[:40, :60]
    d1, d2 = (y - 20) ** 2 + (x - 22) ** 2, (y - 20) ** 2 + (x - 36) ** 2
    sem = ((d1 <= 100) | (d2 <= 100)).astype(np.uint8)
    truth = np.where(sem != 0, np.where(d1 <= d2, 1, 2), 0).astype(np.int32)
    return sem, truth
