"""Shared cases of the surface-metric tests, and their yardstick.

THE YARDSTICK is the recipe MedPy popularised, written with scipy alone in float64: the surface of an object A is
``A ^ binary_erosion(A, generate_binary_structure(dims, 1 or dims))`` (``border_value=0``: positions outside the map are not in A), a
directed sample set is ``distance_transform_edt(~other_surface, sampling=)[own_surface]``, then ``np.max``, ``np.percentile``, ``np.mean``
and a count of the samples ``<= tolerance``.  The conventions for empty surfaces are those of ``surface_metrics``' docstring (an empty other
surface makes every sample ``inf``).  ``brute_force`` restates the sample sets differently -- all pairs of surface positions in int64 --
and tests/test_surface_cpu.py shows it equal to the scipy recipe on every case of at most BRUTE_LIMIT positions.

THE CASES are the shapes at which the kernels of csrc/ptb_surface.hip can go wrong, not the workload's: a wave of the border kernel walks
a row in chunks of 256 positions (4 per lane) and a workgroup holds 4 rows; a lane of the sample kernel reads groups of 16 flags, a
workgroup of it owns a segment of at least 4096 positions of one map; the selection works on the four bytes of a key.  Every pattern
has its seed fixed."""
import functools
from collections import namedtuple

import numpy as np

from distance_cases import SPACINGS

BRUTE_LIMIT = 40_000
EXTENTS = (1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257)
TOLERANCES = (0.0, 1.0, 1.5, 2.0)                   # unit spacing: d^2 is an integer, so d <= tol is exact
SPACING_TOLERANCES = (0.9, 2.05, 3.33, 7.77)        # with spacing: no sample of any case within 1e-5 relative of one (asserted below)
KEYS2 = ("directed_hausdorff", "directed_percentile", "mean_surface_distance")
KEYS1 = ("hausdorff", "hausdorff_percentile", "assd")

Case = namedtuple("Case", "pred truth dims labels background connectivity percentile", defaults=(None, 0, None, 95.0))


# ---------------------------------------------------------------------------------------------------------------- patterns
def noise(shape, seed, classes=2):
    return np.random.default_rng(seed).integers(0, classes, shape).astype(np.uint8)


def blobs(shape, seed, classes=3, cell=5):
    """a label map of square cells of ``cell`` positions with random classes, about half of them background"""
    rng = np.random.default_rng(seed)
    grid = [(s + cell - 1) // cell for s in shape]
    low = rng.integers(1, classes + 1, grid) * (rng.random(grid) < 0.5)
    for axis in range(len(shape)):
        low = np.repeat(low, cell, axis=axis)
    return np.ascontiguousarray(low[tuple(slice(0, s) for s in shape)]).astype(np.uint8)


def perturbed(a, seed):
    """``a`` shifted by one or two positions along its last two axes, with a tenth of its cells of 5 dropped"""
    rng = np.random.default_rng(seed)
    out = np.roll(a, (1, 2), axis=(-2, -1))
    drop = rng.random([(s + 4) // 5 for s in a.shape]) < 0.1
    for axis in range(a.ndim):
        drop = np.repeat(drop, 5, axis=axis)
    out[drop[tuple(slice(0, s) for s in a.shape)]] = 0
    return out


def box(shape, *ranges, value=1):
    a = np.zeros(shape, np.uint8)
    a[tuple(slice(lo, hi) for lo, hi in ranges)] = value
    return a


def _cases():
    c = {}
    # objects that touch every edge of the map: neighbours outside the map make border
    c["edges"] = Case(1 - box((20, 23), (5, 9), (6, 15)), 1 - box((20, 23), (11, 17), (3, 8)), 2)
    c["volume_edges"] = Case(1 - box((6, 7, 9), (2, 4), (2, 5), (3, 7)), 1 - box((6, 7, 9), (1, 3), (3, 6), (2, 5)), 3)
    c["one_position_object"] = Case(box((17, 19), (3, 4), (4, 5)), box((17, 19), (10, 11), (12, 13)), 2)
    c["one_position_map"] = Case(np.ones((1, 1), np.uint8), np.ones((1, 1), np.uint8), 2)
    c["volume_one_position_map"] = Case(np.ones((1, 1, 1), np.uint8), np.ones((1, 1, 1), np.uint8), 3)
    c["whole_map"] = Case(np.ones((9, 11), np.uint8), box((9, 11), (2, 7), (3, 9)), 2)
    c["volume_whole_map"] = Case(np.ones((4, 5, 6), np.uint8), box((4, 5, 6), (1, 3), (1, 4), (2, 5)), 3)
    c["volume_depth_one"] = Case(blobs((1, 17, 23), 300), blobs((1, 17, 23), 301), 3, (1, 2))       # slices before and behind lie outside
    for i, n in enumerate(EXTENTS):
        c[f"len{n}_x"] = Case(noise((5, n), 310 + i, 3), noise((5, n), 330 + i, 3), 2, (1, 2))
        c[f"len{n}_y"] = Case(noise((n, 6), 350 + i, 3), noise((n, 6), 370 + i, 3), 2, (1, 2))
        c[f"len{n}_x3"] = Case(noise((2, 3, n), 390 + i), noise((2, 3, n), 410 + i), 3)
        c[f"len{n}_y3"] = Case(noise((2, n, 5), 430 + i), noise((2, n, 5), 450 + i), 3)
        c[f"len{n}_z3"] = Case(noise((n, 3, 5), 470 + i), noise((n, 3, 5), 490 + i), 3)
    c["offset"] = Case(blobs((20, 64), 500), perturbed(blobs((20, 64), 500), 501), 2, (1, 2, 3))
    c["volume_offset"] = Case(blobs((5, 6, 128), 502), perturbed(blobs((5, 6, 128), 502), 503), 3, (1, 2, 3))
    # squared distances pass 2^24: every byte of the select key decides somewhere
    thin_t = box((8, 4300), (2, 6), (4260, 4300))
    thin_t[3, 45] = 1
    c["long_thin"] = Case(box((8, 4300), (2, 6), (0, 40)), thin_t, 2)
    # many equal keys: both order statistics of the interpolation fall in one key
    for pct in (0.0, 50.0, 95.0, 100.0):
        c[f"squares_p{pct:g}"] = Case(box((40, 40), (10, 30), (10, 30)), box((40, 40), (14, 26), (14, 26)), 2, percentile=pct)
    # 9 and 5 samples: (n - 1) * 0.375 is the integer 3 in pred -> truth and 1.5 in truth -> pred
    c["integer_rank"] = Case(box((12, 20), (4, 5), (3, 12)), box((12, 20), (8, 9), (10, 15)), 2, percentile=37.5)
    c["one_sample"] = Case(box((17, 19), (3, 4), (4, 5)), blobs((17, 19), 504), 2, percentile=60.0)
    c["noise_blocks"] = Case(noise((257, 300), 505), noise((257, 300), 506), 2)         # several workgroups contribute partial sums
    # a stack of 3 with K = 3: class 2 is missing in pred of entry 0, in truth of entry 1 and in both of entry 2
    sp, st = np.stack([blobs((21, 45), 510 + i) for i in range(3)]), np.stack([blobs((21, 45), 520 + i) for i in range(3)])
    sp[0][sp[0] == 2] = 0
    st[1][st[1] == 2] = 0
    sp[2][sp[2] == 2] = 0
    st[2][st[2] == 2] = 0
    c["stack"] = Case(sp, st, 2, (1, 2, 3))
    c["stack_objects"] = Case(sp, st, 2)                                                # labels=None
    c["stack_background2"] = Case(sp, st, 2, None, 2)
    c["stack_unheld_class"] = Case(sp, st, 2, (1, 300, -1, 3))                          # values uint8 cannot hold occur nowhere
    # K = 40: more classes than one chunk takes (32), present ones in the first chunk (1, 2) and in the second (33, 34, 40)
    held = np.array([0, 1, 2, 33, 34, 40], np.uint8)
    c["many_classes"] = Case(held[noise((2, 15, 19), 560, 6)], held[noise((2, 15, 19), 561, 6)], 2, tuple(range(1, 41)))
    vp, vt = np.stack([blobs((7, 12, 21), 530 + i) for i in range(2)]), np.stack([blobs((7, 12, 21), 540 + i) for i in range(2)])
    vp[0][vp[0] == 3] = 0
    c["volume_stack"] = Case(vp, vt, 3, (1, 2, 3))
    for conn in (4, 8):
        c[f"blobs_c{conn}"] = Case(blobs((61, 83), 550), perturbed(blobs((61, 83), 550), 551), 2, (1, 2, 3), connectivity=conn)
    for conn in (6, 26):
        c[f"volume_blobs_c{conn}"] = Case(blobs((9, 22, 35), 552), perturbed(blobs((9, 22, 35), 552), 553), 3, (1, 2, 3), connectivity=conn)
    return c


CASES = _cases()
OFFSET_CASES = ("offset", "volume_offset")
SPACING_CASES = ("edges", "volume_edges", "one_position_object", "whole_map", "len257_x", "len65_y3", "len17_z3", "long_thin", "squares_p50", "integer_rank",
                 "noise_blocks", "stack", "stack_objects", "volume_stack", "blobs_c8", "volume_blobs_c26", "volume_depth_one", "many_classes")
DTYPE_CASES = ("stack", "volume_offset", "offset")
BIG_CASES = ("noise_blocks", "long_thin", "volume_blobs_c26")


# ---------------------------------------------------------------------------------------------------------------- yardstick
def _entries(a, dims):
    a = np.asarray(a)
    return a.reshape((-1,) + a.shape[a.ndim - dims:])


def objects(a, labels, background):
    """the K boolean maps of one entry"""
    a = a.astype(np.int64)
    return [a != background] if labels is None else [a == v for v in labels]


def surface(mask, dims, connectivity):
    from scipy.ndimage import binary_erosion, generate_binary_structure

    full = connectivity in (8, 26)
    return mask ^ binary_erosion(mask, generate_binary_structure(dims, dims if full else 1))


def sample_sets(bp, bt, sampling):
    """the two directed float64 sample sets of a pair of surfaces (scipy)"""
    from scipy.ndimage import distance_transform_edt

    out = []
    for own, other in ((bp, bt), (bt, bp)):
        out.append(distance_transform_edt(~other, sampling=sampling)[own] if other.any() else np.full(int(own.sum()), np.inf))
    return out


def brute_force(bp, bt):
    """the two directed int64 sets of SQUARED index distances, all pairs of surface positions; -1 for "no surface on the other side\""""
    out = []
    for own, other in ((bp, bt), (bt, bp)):
        p, s = np.argwhere(own).astype(np.int64), np.argwhere(other).astype(np.int64)
        if not len(s):
            out.append(np.full(len(p), -1, np.int64))
            continue
        best = np.full(len(p), np.iinfo(np.int64).max)
        step = max(1, 2_000_000 // max(1, len(p)))
        for k in range(0, len(s), step):
            off = p[:, None, :] - s[None, k:k + step, :]
            best = np.minimum(best, (off * off).sum(axis=2).min(axis=1))
        out.append(best)
    return out


def percentile(d, pct):
    """``np.percentile``; a set of infinite samples (the other surface is empty) gives inf"""
    if not len(d):
        return np.nan
    return np.inf if np.isinf(d).any() else np.percentile(d, pct)


def yardstick(case, spacing=None, tolerances=TOLERANCES):
    """dict of float64 arrays shaped like the results of ``surface_metrics`` (no stack dimensions merged: [B, K, ...]), plus ``"within"``
    [B, K, T] int64, the numerator of surface Dice, and with unit spacing ``"max_squared"`` [B, K, 2] int64 (-1: nan or inf)"""
    dims = case.dims
    conn = case.connectivity or (4 if dims == 2 else 6)
    sampling = None if spacing is None else spacing[-dims:]
    P, Tr = _entries(case.pred, dims), _entries(case.truth, dims)
    B, K, T = len(P), 1 if case.labels is None else len(case.labels), len(tolerances)
    res = {"surface_count": np.zeros((B, K, 2), np.int64), "within": np.zeros((B, K, T), np.int64), "surface_dice": np.full((B, K, T), np.nan),
           "max_squared": np.full((B, K, 2), -1, np.int64)}
    res.update({k: np.full((B, K, 2), np.nan) for k in KEYS2})
    res.update({k: np.full((B, K), np.nan) for k in KEYS1})
    samples = []
    for b in range(B):
        for k, (op, ot) in enumerate(zip(objects(P[b], case.labels, case.background), objects(Tr[b], case.labels, case.background))):
            bp, bt = surface(op, dims, conn), surface(ot, dims, conn)
            sets = sample_sets(bp, bt, sampling)
            n = np.array([len(s) for s in sets])
            res["surface_count"][b, k] = n
            for side, d in enumerate(sets):
                if len(d):
                    res["directed_hausdorff"][b, k, side] = d.max()
                    res["directed_percentile"][b, k, side] = percentile(d, case.percentile)
                    res["mean_surface_distance"][b, k, side] = np.mean(d)
                    if spacing is None and np.isfinite(d.max()):
                        res["max_squared"][b, k, side] = int(np.rint(d * d).max())
                samples.append(d[np.isfinite(d)])
            if not n.any():
                continue
            pooled = np.concatenate(sets)
            res["within"][b, k] = [(pooled <= tol).sum() for tol in tolerances]
            res["surface_dice"][b, k] = res["within"][b, k] / float(n.sum())
            res["hausdorff_percentile"][b, k] = percentile(pooled, case.percentile)
            if n.all():
                res["hausdorff"][b, k] = pooled.max()
                res["assd"][b, k] = (np.mean(sets[0]) + np.mean(sets[1])) / 2
            else:
                res["hausdorff"][b, k] = res["assd"][b, k] = np.inf
    res["samples"] = np.concatenate(samples) if samples else np.zeros(0)
    for v in res.values():
        v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def expected(name, spacing=None):
    """the yardstick of a case, computed once per session and shared; with ``spacing`` the tolerances are SPACING_TOLERANCES, and no sample
    may lie within 1e-5 relative of one of them: a count can then differ from the yardstick's only through a bug"""
    res = yardstick(CASES[name], spacing, TOLERANCES if spacing is None else SPACING_TOLERANCES)
    if spacing is not None:
        d = res["samples"]
        for tol in SPACING_TOLERANCES:
            assert not (np.abs(d - tol) <= 1e-5 * tol).any(), (name, spacing, tol)
    return res


def _check_long_thin():
    """the long thin map must reach squared distances past 2^24 (the top byte of the key) next to small ones"""
    c = CASES["long_thin"]
    sq = np.concatenate(brute_force(surface(c.pred != 0, 2, 4), surface(c.truth != 0, 2, 4)))
    assert sq.max() > 1 << 24 and sq.min() < 1 << 8, (sq.max(), sq.min())


_check_long_thin()
