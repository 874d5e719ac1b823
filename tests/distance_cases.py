"""Shared cases of the distance-transform tests, and a restatement of the transform that is written differently from the product's host
form (which takes minima shift by shift, axis by axis): an all-pairs brute force in int64, the minimum over the sites of the summed
squared index offsets, in chunks.  It is the expected value of every case of at most BRUTE_LIMIT positions; for the larger ones the
expected value is scipy's (``rint(distance_transform_edt(x) ** 2)``), which tests/test_distance_cpu.py shows to equal the brute force
on every small case.  An entry without a site is expected to be INF = 2^31 - 1 (float forms: inf).

A case is a label map whose zeros are the sites (``background=0``).  The maps of tests/components_cases.py are all here; added are the
shapes at which the kernels of csrc/ptb_distance.hip can go wrong.  Their constants: a wave of the row pass walks its row in chunks
of CHUNK = 256 positions (64 lanes x 4), a wave of the line passes holds WAVE = 64 neighbouring lines -- hence line lengths 1, 2,
WAVE - 1, WAVE, WAVE + 1, 2 WAVE + 1, CHUNK - 1, CHUNK, CHUNK + 1 along every axis of both ``dims``.  Every pattern has its seed fixed."""
import functools

import numpy as np

import components_cases as C

WAVE = 64
CHUNK = 256
LENGTHS = (1, 2, WAVE - 1, WAVE, WAVE + 1, 2 * WAVE + 1, CHUNK - 1, CHUNK, CHUNK + 1)
INF = (1 << 31) - 1
BRUTE_LIMIT = 40_000
SPACINGS = ((2.5, 0.7, 0.7), (1.0, 1.0, 3.0))           # the last `dims` entries are used


# ---------------------------------------------------------------------------------------------------------------- patterns
def sparse(shape, seed, p=0.08):
    """mostly object, a few sites"""
    return (np.random.default_rng(seed).random(shape) >= p).astype(np.uint8)


def one_site(shape, at):
    a = np.ones(shape, np.uint8)
    a[tuple(at)] = 0
    return a


def one_object(shape, at):
    a = np.zeros(shape, np.uint8)
    a[tuple(at)] = 1
    return a


def stripes(shape, axis, at):
    """sites are the whole hyperplanes ``at`` across ``axis``: everything between them has no site of its own along the other axes"""
    a = np.ones(shape, np.uint8)
    idx = [slice(None)] * len(shape)
    idx[axis] = list(at)
    a[tuple(idx)] = 0
    return a


def _cases():
    c = {name: (a, dims) for name, (a, dims) in C.CASES.items()}
    for i, n in enumerate(LENGTHS):
        c[f"len{n}_x"] = (sparse((5, n), 100 + i), 2)
        c[f"len{n}_y"] = (sparse((n, 6), 120 + i), 2)
        c[f"len{n}_x3"] = (sparse((2, 3, n), 140 + i), 3)
        c[f"len{n}_y3"] = (sparse((2, n, 5), 160 + i), 3)
        c[f"len{n}_z3"] = (sparse((n, 3, 5), 180 + i), 3)
    c["one_site"] = (C.zeros((1, 1)), 2)
    c["depth_one"] = (sparse((1, 17, 23), 200), 3)
    c["sparse_W%4"] = (sparse((21, CHUNK + 3), 201, p=0.01), 2)
    c["sparse_offset"] = (sparse((20, WAVE), 202, p=0.02), 2)
    c["volume_sparse_offset"] = (sparse((5, 6, 2 * WAVE), 203, p=0.01), 3)
    for k, (y, x) in enumerate(((0, 0), (0, -1), (-1, 0), (-1, -1))):
        c[f"corner{k}"] = (one_site((37, 70), (y, x)), 2)
    for k in range(8):
        c[f"volume_corner{k}"] = (one_site((5, 12, 70), (-(k >> 2 & 1), -(k >> 1 & 1), -(k & 1))), 3)
    c["one_object"] = (one_object((33, 67), (16, 40)), 2)
    c["volume_one_object"] = (one_object((5, 9, 67), (2, 3, 65)), 3)
    c["stripes_y"] = (stripes((40, 30), 0, (10, 25)), 2)                      # rows without a site at the start, in the middle, at the end
    c["stripes_x"] = (stripes((30, 70), 1, (9, 66)), 2)
    points = np.ones((40, 70), np.uint8)
    points[10, 3] = points[25, 68] = points[26, 0] = 0
    c["stripes_y_points"] = (points, 2)                                       # ... and different values in the rows that have one
    c["stripes_z"] = (stripes((12, 14, 20), 0, (3, 9)), 3)                    # whole slices without a site
    c["stripes_y3"] = (stripes((6, 21, 20), 1, (5, 6, 15)), 3)
    c["stripes_x3"] = (stripes((6, 7, 70), 2, (0, 40)), 3)
    vpoints = np.ones((12, 9, 20), np.uint8)
    vpoints[3, 2, 5] = vpoints[9, 8, 19] = vpoints[10, 0, 0] = 0
    c["stripes_z_points"] = (vpoints, 3)
    c["stack_hole"] = (np.stack([sparse((21, 45), 204), C.ones((21, 45)), sparse((21, 45), 205, p=0.01)]), 2)      # carries must not leak
    c["volume_stack_hole"] = (np.stack([sparse((5, 9, 21), 206), C.ones((5, 9, 21)), sparse((5, 9, 21), 207, p=0.01)]), 3)
    c["wide_one_site"] = (one_site((300, 1500), (17, 23)), 2)                 # squared distances up to 2.3e6: sqrtf on large arguments
    c["volume_big"] = (C.blobs((33, 65, 130), 208, classes=4, cell=9), 3)
    return c


CASES = _cases()
OFFSET_CASES = C.OFFSET_CASES + ("sparse_offset", "volume_sparse_offset")
BIG_CASES = C.BIG_CASES + ("wide_one_site", "volume_big")
FOREGROUND_CASES = ("blobs", "noise4_wide", "touching")
SIGNED_CASES = tuple(n for n in CASES if n != "volume_blobs")                # (its complement has 29 000 sites: 20 s of brute force)
SPACING_CASES = ("blobs", "noise_2T+1", "speckle", "stack", "corner1", "corner2", "stripes_y_points", "stack_hole", "len257_x", "len257_y", "wide_one_site",
                 "spiral_big", "volume_blobs", "volume_noise_2T+1", "volume_corner3", "volume_corner6", "stripes_z_points", "stripes_y3", "volume_stack_hole",
                 "len257_z3", "len65_y3", "volume_big")


# ---------------------------------------------------------------------------------------------------------------- restatement
def _entries(a, dims):
    a = np.asarray(a)
    return a.reshape((-1,) + a.shape[a.ndim - dims:])


def brute_force(sites, dims):
    """int64 squared distance of every position to the nearest True of ``sites`` ([*stack, (D,) H, W]) within its entry; INF without one"""
    sites = np.asarray(sites, dtype=bool)
    out = np.full(_entries(sites, dims).shape, INF, np.int64)
    for e, o in zip(_entries(sites, dims), out):
        s = np.argwhere(e).astype(np.int64)
        if not len(s):
            continue
        p = np.argwhere(np.ones(e.shape, bool)).astype(np.int64)
        step = max(1, 4_000_000 // len(p))
        best = np.full(len(p), np.iinfo(np.int64).max)
        for k in range(0, len(s), step):
            d = np.zeros((len(p), len(s[k:k + step])), np.int64)
            for axis in range(dims):
                off = p[:, axis, None] - s[None, k:k + step, axis]
                d += off * off
            best = np.minimum(best, d.min(axis=1))
        o[...] = best.reshape(e.shape)
    return out.reshape(sites.shape)


def scipy_squared(sites, dims, sampling=None):
    """scipy's squared distances per entry: int64 ``rint(d ** 2)`` (INF without a site), or with ``sampling`` float64 ``d ** 2`` (inf)"""
    from scipy.ndimage import distance_transform_edt

    sites = np.asarray(sites, dtype=bool)
    ent = _entries(sites, dims)
    out = np.full(ent.shape, INF if sampling is None else np.inf, np.int64 if sampling is None else np.float64)
    for e, o in zip(ent, out):
        if e.any():
            d = distance_transform_edt(~e, sampling=sampling)
            o[...] = np.rint(d * d).astype(np.int64) if sampling is None else d * d
    return out.reshape(sites.shape)


def restate(sites, dims):
    return brute_force(sites, dims) if np.asarray(sites).size <= BRUTE_LIMIT else scipy_squared(sites, dims)


@functools.lru_cache(maxsize=None)
def expected(name, complement=False):
    """The exact squared distances (int64, INF without a site) of a case to its sites (the zeros), or with ``complement`` to its object
    positions; computed once per session and shared."""
    a, dims = CASES[name]
    out = restate((a != 0) if complement else (a == 0), dims)
    out.setflags(write=False)
    return out


def expected_signed(name):
    """int64: expected(object) - expected(sites)"""
    return expected(name, True) - expected(name)


@functools.lru_cache(maxsize=None)
def expected_spacing(name, spacing, complement=False):
    """float64 squared distances under ``spacing`` (scipy's ``sampling=``), inf without a site"""
    a, dims = CASES[name]
    out = scipy_squared((a != 0) if complement else (a == 0), dims, sampling=spacing[-dims:])
    out.setflags(write=False)
    return out


def as_float(sq):
    """float64 distances of exact squared ones"""
    return np.where(sq >= INF, np.inf, np.sqrt(np.where(sq >= INF, 0, sq).astype(np.float64)))
