"""Shared cases of the skeleton tests, and THE DIRECT STATEMENT of the definitions of utils/skeleton.py: one entry at a time, the eight
neighbours as integer arrays cut from a zero-padded copy, ``B``, ``A``, ``C``, ``N1``, ``N2`` as integer sums and the conditions as comparisons --
no words, no bit algebra, not the product's host form.  Expectations are computed once per session.

Known answers (checked with this model): see ``KNOWN``."""
import functools

import numpy as np
from scipy import ndimage

METHODS = ("zhang", "guo_hall")
RELAX_BATCH = 8                     # csrc/ptb_relax_device.h: the launches between two read-backs
STEPS = 32                          # csrc/ptb_skeleton.hip: the sub-iterations of one launch


# ---------------------------------------------------------------------------------------------------------------- the model
def deleted(s, method, k):
    """the positions of the 0/1 map ``s`` [H, W] that sub-iteration ``k`` of ``method`` deletes"""
    H, W = s.shape
    p = np.zeros((H + 2, W + 2), np.int8)
    p[1:-1, 1:-1] = s
    at = {2: (-1, 0), 3: (-1, 1), 4: (0, 1), 5: (1, 1), 6: (1, 0), 7: (1, -1), 8: (0, -1), 9: (-1, -1)}
    P = {i: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for i, (dy, dx) in at.items()}
    cycle = [2, 3, 4, 5, 6, 7, 8, 9, 2]
    if method == "zhang":
        B = sum(P[i] for i in range(2, 10))
        A = sum((P[i] == 0) & (P[j] == 1) for i, j in zip(cycle[:-1], cycle[1:]))
        if k == 0:
            cond = (P[2] * P[4] * P[6] == 0) & (P[4] * P[6] * P[8] == 0)
        else:
            cond = (P[2] * P[4] * P[8] == 0) & (P[2] * P[6] * P[8] == 0)
        return (s == 1) & (B >= 2) & (B <= 6) & (A == 1) & cond
    no = {i: 1 - P[i] for i in P}
    C = (no[2] & (P[3] | P[4])) + (no[4] & (P[5] | P[6])) + (no[6] & (P[7] | P[8])) + (no[8] & (P[9] | P[2]))
    N1 = (P[9] | P[2]) + (P[3] | P[4]) + (P[5] | P[6]) + (P[7] | P[8])
    N2 = (P[2] | P[3]) + (P[4] | P[5]) + (P[6] | P[7]) + (P[8] | P[9])
    N = np.minimum(N1, N2)
    m = ((P[6] | P[7] | no[9]) & P[8]) if k == 0 else ((P[2] | P[3] | no[5]) & P[4])
    return (s == 1) & (C == 1) & (N >= 2) & (N <= 3) & (m == 0)


def thin(mask, method, max_iterations=None):
    """``(skeleton bool, iteration count)`` of one entry"""
    s = mask.astype(np.int8)
    done = 0
    while max_iterations is None or done < max_iterations:
        before = s.sum()
        for k in (0, 1):
            s = np.where(deleted(s, method, k), np.int8(0), s)
        if s.sum() == before:
            break
        done += 1
    return s.astype(bool), done


def model(mask, method, max_iterations=None):
    """``(skeleton, the count of the entry that took longest)`` of a map or a stack of maps"""
    if mask.ndim == 2:
        return thin(mask, method, max_iterations)
    parts = [model(m, method, max_iterations) for m in mask]
    return np.stack([p[0] for p in parts]), max([p[1] for p in parts], default=0)


def components(mask):
    return ndimage.label(mask, structure=np.ones((3, 3)))[1]


def holes(mask):
    """the 4-connected components of the padded complement, less the outside"""
    return ndimage.label(~np.pad(mask, 1))[1] - 1


def cldice_model(pred, truth, values, method):
    """``(counts int64 [*stack, K, 4], cldice, tprec, tsens float32 [*stack, K])``; ``values``: the class values, or None for "not 0\""""
    stack = pred.shape[:-2]
    K = 1 if values is None else len(values)
    counts = np.zeros(stack + (K, 4), np.int64)
    for at in np.ndindex(*stack):
        for k in range(K):
            vp, vt = (pred[at] != 0, truth[at] != 0) if values is None else (pred[at] == values[k], truth[at] == values[k])
            sp, st = thin(vp, method)[0], thin(vt, method)[0]
            counts[at + (k,)] = [(sp & vt).sum(), sp.sum(), (st & vp).sum(), st.sum()]
    c = counts.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        tprec, tsens = c[..., 0] / c[..., 1], c[..., 2] / c[..., 3]
        cl = 2 * tprec * tsens / (tprec + tsens)
    empty_p, empty_t = counts[..., 1] == 0, counts[..., 3] == 0
    cl[(empty_p != empty_t) | (~empty_p & ~empty_t & (tprec + tsens == 0))] = 0.0
    cl[empty_p & empty_t] = np.nan
    return counts, cl.astype(np.float32), tprec.astype(np.float32), tsens.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the cases
def _build():
    rng = np.random.default_rng(0)
    c = {}
    c["blobs"] = ndimage.gaussian_filter(rng.random((150, 170)), 4) > 0.5
    c["noise"] = rng.random((90, 110)) > 0.5
    c["full"] = np.ones((70, 130), bool)
    sq2 = np.zeros((6, 5), bool)
    sq2[2:4, 1:3] = True
    c["sq2"] = sq2
    bar = np.zeros((9, 20), bool)
    bar[3:6, 2:18] = True
    c["bar"] = bar
    yy, xx = np.mgrid[:140, :140]
    r = np.hypot(yy - 70, xx - 70)                          # (an odd disc: zhang deletes one that shrinks to a 2 x 2 square)
    c["rings"] = (r < 8) | ((r > 16) & (r < 27)) | ((r > 36) & (r < 44)) | ((r > 55) & (r < 68))
    # widths and heights around the word, the tile and the row of words; objects on every border
    for H, W in ((1, 33), (63, 31), (64, 32), (65, 65), (64, 64), (20, 5), (33, 110)):
        m = ndimage.gaussian_filter(np.random.default_rng(H * 1000 + W).random((H, W)), 2) > 0.48
        m[0, :] = m[-1, :] = True
        m[:, 0] = m[:, -1] = True
        c[f"border_{H}x{W}"] = m
    yy, xx = np.mgrid[:130, :130]
    c["diagonal"] = np.abs(yy - xx) <= 1                       # 2-thick steps through the tile corner (64, 64)
    seams = np.zeros((130, 130), bool)
    seams[60:68, :] = True                                     # across rows 63 / 64
    seams[:, 60:68] = True                                     # across columns 63 / 64
    seams[:, 28:36] = True                                     # across the word seam 31 / 32
    c["seams"] = seams
    retire = np.zeros((70, 200), bool)                         # small blobs in one tile, a 60-thick square in another: tiles retire at different launches
    retire[:, :64] = ndimage.gaussian_filter(np.random.default_rng(3).random((70, 64)), 2) > 0.52
    retire[4:64, 132:192] = True
    c["retire"] = retire
    stack = np.zeros((3, 40, 50), bool)                        # entries that need different iteration counts
    stack[0] = True
    stack[1, 18:22, 5:45] = True
    c["stack"] = stack
    edge = 2 * RELAX_BATCH * STEPS + STEPS + 6                  # a full square is peeled in about edge sub-iterations: more than two batches of launches
    c["three_batches"] = np.ones((edge, edge), bool)
    return c


CASES = _build()
NAMES = tuple(CASES)
PROPERTY_CASES = ("blobs", "rings", "bar", "full")             # both methods: subset, idempotent, components and holes kept
# name -> method -> (iterations or None, skeleton positions)
KNOWN = {"blobs": {"zhang": (12, 1252), "guo_hall": (14, 1197)}, "full": {"zhang": (35, 60), "guo_hall": (35, 61)},
         "sq2": {"zhang": (1, 0), "guo_hall": (1, 1)}, "bar": {"zhang": (None, 13), "guo_hall": (None, 14)}}


@functools.lru_cache(maxsize=None)
def expected(name, method, max_iterations=None):
    skel, n = model(CASES[name], method, max_iterations)
    skel.setflags(write=False)
    return skel, n
