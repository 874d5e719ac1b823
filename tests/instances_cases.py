"""Shared cases of the instance-matching tests, and their yardstick.

THE YARDSTICK is the numpy recipe a user would write on the host, independent of the product's host form (which sorts the fused keys
and cuts the sorted list into runs): ``np.unique(key, return_index=True, return_counts=True)`` ordered by the first index, ``np.bincount``
areas, IoU = I / (A_p + A_t - I) in float64, a match iff IoU > threshold (and equal classes inside ``0 .. K - 1``), ``math.fsum`` for the IoU
sums.  tests/test_instances_cpu.py cross-checks its table against ``sklearn.metrics.cluster.contingency_matrix(sparse=True)``.

THE CASES are the shapes at which csrc/ptb_instances.hip can go wrong, not the workload's: a workgroup of the pair kernel owns a chunk
of 1024 consecutive positions, four per lane, read with one 16-byte load per map when both bases are aligned; its LDS tables have 1024
slots; the rows are numbered through a bitmap word per 32 positions and a scan whose tile is 2048 words (65 536 positions).  Instance
maps come from the flood fill of components_cases.py or are built by hand, never from the code under test.  Every pattern has its
seed fixed."""
import functools
import math
from collections import namedtuple

import numpy as np

import components_cases as CC

THRESHOLDS = (0.5, 0.75, 0.9)
NUM_CLASSES = 5                                     # label values 1 .. 4 serve as classes; class 0 has no instance
Case = namedtuple("Case", "pred truth n_pred n_truth class_pred class_truth offset", defaults=(False,))


# ---------------------------------------------------------------------------------------------------------------- patterns
def label_blobs(shape, seed, classes=4, cell=12):
    """a label map of square cells of ``cell`` positions with random classes 1 .. classes, about half of them background"""
    rng = np.random.default_rng(seed)
    grid = [(s + cell - 1) // cell for s in shape]
    low = rng.integers(1, classes + 1, grid) * (rng.random(grid) < 0.5)
    for axis in range(len(shape)):
        low = np.repeat(low, cell, axis=axis)
    return np.ascontiguousarray(low[tuple(slice(0, s) for s in shape)]).astype(np.uint8)


def _flood(labels):
    """(instance map int32, n, class of every instance) by the tests' flood fill, all neighbours"""
    dims = labels.ndim
    r = CC.restate(labels, dims, 8 if dims == 2 else 26)
    return r["cc"].astype(np.int32), int(r["count"]), r["values"][0].astype(np.int64), r["areas"][0]


def perturbed_labels(labels, classes=4):
    """``labels`` shifted by (1, 2) along its last two axes, with one blob removed, the largest blob given another class (its partner is
    rejected only for its class) and one blob of 3 x 3 added where both maps are background"""
    t = np.zeros_like(labels)
    t[..., 1:, 2:] = labels[..., :-1, :-2]
    cc, n, _, areas = _flood(t)
    if n >= 3:
        big = int(np.argmax(areas)) + 1
        gone = 1 if big != 1 else 2
        t[cc == gone] = 0
        t[cc == big] = t[cc == big][0] % classes + 1
    free = (labels == 0) & (t == 0)
    for pos in np.argwhere(free):
        window = tuple(slice(int(v), int(v) + 1) for v in pos[:-2]) + (slice(int(pos[-2]), int(pos[-2]) + 3), slice(int(pos[-1]), int(pos[-1]) + 3))
        if free[window].size == 9 and free[window].all():
            t[window] = 1
            break
    return t


def labels_pair(labels, offset=False):
    truth_labels = perturbed_labels(labels)
    p, n_p, cls_p, _ = _flood(labels)
    t, n_t, cls_t, _ = _flood(truth_labels)
    return Case(p, t, n_p, n_t, cls_p, cls_t, offset), labels, truth_labels


def by_hand(pred, truth, n_pred=None, n_truth=None):
    pred, truth = np.asarray(pred, np.int32), np.asarray(truth, np.int32)
    n_p = int(max(pred.max(), 0)) if n_pred is None else n_pred
    n_t = int(max(truth.max(), 0)) if n_truth is None else n_truth
    return Case(pred, truth, n_p, n_t, np.arange(1, n_p + 1, dtype=np.int64) % 3 + 1, np.arange(1, n_t + 1, dtype=np.int64) % 3 + 1)


def _noise_pair():
    rng = np.random.default_rng(31)
    a = rng.integers(0, 4, (96, 160)).astype(np.uint8)
    b = a.copy()
    change = rng.random(a.shape) < 0.08
    b[change] = rng.integers(0, 4, int(change.sum()))
    p, n_p, cls_p, _ = _flood(a)
    t, n_t, cls_t, _ = _flood(b)
    return Case(p, t, n_p, n_t, cls_p, cls_t), a, b


def _giant_pair():
    pred = np.ones((64, 64), np.int32)
    truth = np.zeros((64, 64), np.int32)
    truth[::2, ::2] = np.arange(1, 1025, dtype=np.int32).reshape(32, 32)
    return by_hand(pred, truth)


def _long_run():
    pred, truth = np.zeros((1, 5000), np.int32), np.zeros((1, 5000), np.int32)
    pred[0, 100:4700] = 1
    pred[0, 4700:4990] = 2
    truth[0, 50:4600] = 1
    truth[0, 4600:4900] = 2
    return by_hand(pred, truth)


def _foreign_ids():
    """ids above n and negative ids: background"""
    case = _blob_pair()[0]
    pred, truth = case.pred.copy(), case.truth.copy()
    pred[0, :7] = -3
    pred[5, 10:14] = case.n_pred + 5
    truth[-1, -6:] = -(2 ** 31)
    truth[truth == case.n_truth] = 2 ** 31 - 1
    n_p, n_t = case.n_pred - 2, case.n_truth - 1          # the last ids of both sides are above n now
    return Case(pred, truth, n_p, n_t, case.class_pred[:n_p], case.class_truth[:n_t])


@functools.lru_cache(maxsize=None)
def _blob_pair():
    return labels_pair(label_blobs((37, 53), 3))


@functools.lru_cache(maxsize=None)
def _cases():
    c = {}
    c["one"] = by_hand([[1]], [[1]])
    c["iou_half"] = by_hand([[1, 1, 1, 0, 0, 0, 0]], [[0, 1, 1, 1, 0, 0, 0]])                 # A_p = 3, A_t = 3, I = 2: IoU is exactly 0.5
    c["iou_three_quarters"] = by_hand([[1, 1, 1, 1, 0, 0, 0]], [[1, 1, 1, 0, 0, 0, 0]])       # A_p = 4, A_t = 3, I = 3: exactly 0.75
    c["small"] = by_hand([[1, 1, 0, 2, 2], [1, 1, 0, 2, 2], [3, 3, 3, 0, 0]], [[1, 1, 1, 2, 2], [0, 1, 0, 0, 2], [3, 3, 0, 0, 4]])
    c["chunk"] = labels_pair(label_blobs((32, 32), 5, cell=6))[0]                              # 1024 positions exactly
    c["chunk+1"] = labels_pair(label_blobs((25, 41), 6, cell=6))[0]                            # 1025
    c["blobs"] = _blob_pair()[0]
    c["blobs_offset"] = _blob_pair()[0]._replace(offset=True)
    c["noise"] = _noise_pair()[0]
    c["giant"] = _giant_pair()
    zeros = np.zeros((20, 30), np.int32)
    some = labels_pair(label_blobs((20, 30), 7, cell=6))[0]
    c["empty_both"] = by_hand(zeros, zeros)
    c["empty_pred"] = Case(zeros, some.truth, 0, some.n_truth, np.zeros(0, np.int64), some.class_truth)
    c["empty_truth"] = Case(some.pred, zeros, some.n_pred, 0, some.class_pred, np.zeros(0, np.int64))
    c["long_run"] = _long_run()
    c["foreign_ids"] = _foreign_ids()
    c["blobs_big"] = labels_pair(label_blobs((300, 400), 8, cell=14))[0]                       # 3751 bitmap words: two tiles of the scan
    c["volume"] = labels_pair(label_blobs((24, 40, 56), 9, cell=13))[0]
    return c


def names():
    return tuple(_cases())


def case(name):
    return _cases()[name]


def chain_labels():
    """the two label maps behind the ``blobs`` case: what the chain test hands to connected_components"""
    _, a, b = _blob_pair()
    return a, b


# ---------------------------------------------------------------------------------------------------------------- yardstick
def _clamp(ids, n):
    a = np.asarray(ids).reshape(-1).astype(np.int64)
    a[(a < 1) | (a > n)] = 0
    return a


def table(pred, truth, n_pred, n_truth):
    """dict(pairs [P, 2] int32 in first-position order, intersection [P], pred_area, truth_area)"""
    p, t = _clamp(pred, n_pred), _clamp(truth, n_truth)
    key = p * (n_truth + 1) + t
    key[(p == 0) | (t == 0)] = 0
    uniq, first, counts = np.unique(key, return_index=True, return_counts=True)
    keep = uniq > 0
    uniq, first, counts = uniq[keep], first[keep], counts[keep]
    order = np.argsort(first)
    pairs = np.stack(np.divmod(uniq[order], n_truth + 1), axis=1).astype(np.int32).reshape(-1, 2)
    return dict(pairs=pairs, intersection=counts[order].astype(np.int64), pred_area=np.bincount(p, minlength=n_pred + 1)[1:].astype(np.int64),
                truth_area=np.bincount(t, minlength=n_truth + 1)[1:].astype(np.int64))


def match(pred, truth, n_pred, n_truth, thresholds=THRESHOLDS, class_pred=None, class_truth=None, num_classes=0):
    """what match_instances returns, as numpy arrays ([T] without classes, [K, T] with)"""
    tab = table(pred, truth, n_pred, n_truth)
    ap_, at_ = tab["pred_area"], tab["truth_area"]
    res = dict(pred_match=np.zeros(n_pred, np.int32), truth_match=np.zeros(n_truth, np.int32), pred_iou=np.zeros(n_pred), truth_iou=np.zeros(n_truth),
               pred_area=ap_, truth_area=at_, num_pairs=np.int64(len(tab["pairs"])))
    rejected_for_class = 0
    for (p, t), inter in zip(tab["pairs"].tolist(), tab["intersection"].tolist()):
        iou = np.float64(inter) / np.float64(ap_[p - 1] + at_[t - 1] - inter)
        if not iou > thresholds[0]:
            continue
        if num_classes and not (class_pred[p - 1] == class_truth[t - 1] and 0 <= class_pred[p - 1] < num_classes):
            rejected_for_class += 1
            continue
        res["pred_match"][p - 1], res["truth_match"][t - 1], res["pred_iou"][p - 1], res["truth_iou"][t - 1] = t, p, iou, iou
    K, T = max(num_classes, 1), len(thresholds)
    for key in ("tp", "fp", "fn"):
        res[key] = np.zeros((K, T), np.int64)
    for key in ("sum_iou", "sq", "rq", "pq", "ap"):
        res[key] = np.full((K, T), np.nan)
    for k in range(K):
        in_p = np.ones(n_pred, bool) if not num_classes else np.asarray(class_pred) == k
        in_t = np.ones(n_truth, bool) if not num_classes else np.asarray(class_truth) == k
        for j, tau in enumerate(thresholds):
            hit = in_p & (res["pred_iou"] > tau)
            tp, s = int(hit.sum()), math.fsum(res["pred_iou"][hit].tolist())
            fp, fn = int((in_p & (ap_ > 0)).sum()) - tp, int((in_t & (at_ > 0)).sum()) - tp
            res["tp"][k, j], res["fp"][k, j], res["fn"][k, j], res["sum_iou"][k, j] = tp, fp, fn, s
            half = tp + fp / 2 + fn / 2
            if tp:
                res["sq"][k, j] = s / tp
            if half:
                res["rq"][k, j], res["pq"][k, j] = tp / half, s / half
            if tp + fp + fn:
                res["ap"][k, j] = tp / (tp + fp + fn)
    if not num_classes:
        for key in ("tp", "fp", "fn", "sum_iou", "sq", "rq", "pq", "ap"):
            res[key] = res[key][0]
    res["rejected_for_class"] = rejected_for_class
    return res


@functools.lru_cache(maxsize=None)
def expected_table(name):
    c = case(name)
    return table(c.pred, c.truth, c.n_pred, c.n_truth)


@functools.lru_cache(maxsize=None)
def expected(name, classes=False, thresholds=THRESHOLDS):
    """match() of a case, computed once per session and shared"""
    c = case(name)
    if classes:
        return match(c.pred, c.truth, c.n_pred, c.n_truth, thresholds, c.class_pred, c.class_truth, NUM_CLASSES)
    return match(c.pred, c.truth, c.n_pred, c.n_truth, thresholds)


# ---------------------------------------------------------------------------------------------------------------- comparison
INTEGER_KEYS = ("pred_match", "truth_match", "pred_area", "truth_area", "tp", "fp", "fn", "num_pairs")
SUMMED_KEYS = ("sum_iou", "sq", "rq", "pq", "ap")


def assert_matches(got, want, n_pred, context):
    """integers, match arrays and the float64 IoUs bit-equal; sum_iou and the scores within n_pred * 2^-52 relative of the math.fsum
    values: the bound of an n-term double sum of values in [0, 1] (the divisions add at most one rounding of the same size)"""
    got = {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in got.items()}
    for key in INTEGER_KEYS:
        assert got[key].dtype == np.asarray(want[key]).dtype and got[key].shape == np.shape(want[key]), (context, key, got[key].dtype, got[key].shape)
        assert np.array_equal(got[key], want[key]), (context, key, got[key], want[key])
    for key in ("pred_iou", "truth_iou"):
        assert got[key].dtype == np.float64 and np.array_equal(got[key].view(np.int64), want[key].view(np.int64)), (context, key)
    bound = max(n_pred, 1) * 2.0 ** -52
    for key in SUMMED_KEYS:
        g, w = got[key], want[key]
        assert g.dtype == np.float64 and g.shape == w.shape, (context, key, g.shape, w.shape)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (context, key, g, w)
        ok = ~np.isnan(w)
        assert np.all(np.abs(g[ok] - w[ok]) <= bound * np.abs(w[ok])), (context, key, g, w)
