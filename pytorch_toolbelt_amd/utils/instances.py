"""Object-level scores of two instance maps, on the device the tensors are on: the overlap table between the instances of a prediction
and those of the ground truth, the one-to-one matching above IoU 0.5 and what instance and panoptic evaluations report from it -- TP / FP /
FN per threshold, panoptic quality (PQ = SQ x RQ), F1 at IoU 0.5, the DSB-2018 / StarDist / Cellpose score ``TP / (TP + FP + FN)``.  It
is the step behind ``connected_components``: label both maps, then score their objects without leaving the device.

The reference has no counterpart, so the names and meanings below are this library's; the numpy recipe ``np.unique`` of fused keys,
``np.bincount`` areas and a float64 IoU is the yardstick.  CUDA tensors run the HIP kernels of ``csrc/ptb_instances.hip`` (a missing kernel
is an error, never a silent host computation), CPU tensors take the numpy form below with the same results -- the device the caller
names decides.

Left out: matching below IoU 0.5 (an assignment problem), best-overlap scores such as AJI, the void / crowd regions of the COCO panoptic
protocol, stacks in one call, and maps in other dtypes than int32.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _native as N
from . import _maps as M

__all__ = ["instance_overlaps", "match_instances"]

MAX_PAIRS = 1 << 28                      # what a call may ask for
DEFAULT_MAX_PAIRS = 1 << 22              # what a call without max_pairs is sized for at most
MAX_THRESHOLDS = 16
MAX_CLASSES = 65535
_OUTPUTS = ("num_pairs", "pred_area", "truth_area", "pairs", "intersection", "pred_match", "truth_match", "pred_iou", "truth_iou", "tp", "fp", "fn",
            "sum_iou", "sq", "rq", "pq", "ap")
_INT32 = ("pairs", "pred_match", "truth_match")
_FLOAT64 = ("pred_iou", "truth_iou", "sum_iou", "sq", "rq", "pq", "ap")
_SCORES = ("sq", "rq", "pq", "ap")
_PER_THRESHOLD = ("tp", "fp", "fn", "sum_iou") + _SCORES


# ---------------------------------------------------------------------------------------------------------------- validation
def _maps(what, pred, truth):
    for name, t in (("pred", pred), ("truth", truth)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.int32:
            raise TypeError(f"{what}: {name} must be an int32 instance map (what connected_components returns), got {t.dtype}")
    if pred.shape != truth.shape:
        raise ValueError(f"{what}: pred and truth must have the same shape, got {tuple(pred.shape)} and {tuple(truth.shape)}")
    if pred.device != truth.device:
        raise ValueError(f"{what}: pred and truth must be on the same device, got {pred.device} and {truth.device}")
    if pred.numel() > M.MAX_POSITIONS:
        raise ValueError(f"{what}: {pred.numel()} positions; at most 2^31 - 2 = {M.MAX_POSITIONS}")


def _count(what, name, v, ids):
    """the ``n`` of one side: an int (nothing is read back), a 0-dim count tensor or None (``ids.max()``): 8 bytes read back"""
    if isinstance(v, torch.Tensor):
        if v.dim() != 0:
            raise ValueError(f"{what}: {name} must be an int, a 0-dim tensor or None, got a tensor of shape {tuple(v.shape)}: one entry per call")
        n = int(v.item())
    elif v is None:
        n = max(int(ids.max().item()), 0) if ids.numel() else 0
    else:
        n = M.check_int(what, name, v)
    if n < 0:
        raise ValueError(f"{what}: {name} is {n}{': the labelling failed' if isinstance(v, torch.Tensor) else '; it must be >= 0'}")
    return min(n, M.MAX_POSITIONS)


def _pairs_cap(what, max_pairs, positions, n_p, n_t):
    """``(m, given)``: the rows the table is sized for"""
    max_pairs = M.check_int(what, "max_pairs", max_pairs, allow_none=True)
    if max_pairs is None:
        return min(positions, n_p * n_t, DEFAULT_MAX_PAIRS), False       # (a pair needs a position, and an id of each side)
    if not 0 <= max_pairs <= MAX_PAIRS:
        raise ValueError(f"{what}: max_pairs must lie in 0 .. 2^28, got {max_pairs}")
    return max_pairs, True


def _thresholds(what, thresholds):
    seq = [thresholds] if isinstance(thresholds, (int, float, np.integer, np.floating)) and not isinstance(thresholds, (bool, np.bool_)) else thresholds
    try:
        taus = [float(t) for t in seq]
    except (TypeError, ValueError):
        raise TypeError(f"{what}: thresholds must be a float or a sequence of 1 to {MAX_THRESHOLDS} floats, got {thresholds!r}") from None
    if not 1 <= len(taus) <= MAX_THRESHOLDS:
        raise ValueError(f"{what}: thresholds must have 1 to {MAX_THRESHOLDS} entries, got {len(taus)}")
    if not all(0.5 <= t < 1.0 for t in taus):                  # (nan fails both comparisons)
        raise ValueError(f"{what}: every threshold must satisfy 0.5 <= t < 1, got {taus}: below 0.5 a match is no longer unique and needs an "
                         "assignment solver")
    if any(b <= a for a, b in zip(taus, taus[1:])):
        raise ValueError(f"{what}: thresholds must increase, got {taus}")
    return taus


def _classes(what, pred_class, truth_class, num_classes, n_p, n_t, dev):
    given = [v is not None for v in (pred_class, truth_class, num_classes)]
    if not any(given):
        return 0
    if not all(given):
        raise ValueError(f"{what}: pred_class, truth_class and num_classes are given together or not at all")
    K = M.check_int(what, "num_classes", num_classes)
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"{what}: num_classes must lie in 1 .. {MAX_CLASSES}, got {K}")
    for name, c, n in (("pred_class", pred_class, n_p), ("truth_class", truth_class, n_t)):
        if not isinstance(c, torch.Tensor) or c.dtype not in M.ELEM_BYTES:
            raise TypeError(f"{what}: {name} must be an integer tensor (bool, uint8, int16, int32 or int64)")
        if tuple(c.shape) != (n,) or c.device != dev:
            raise ValueError(f"{what}: {name} must be of shape ({n},) on {dev} (one class per instance), got {tuple(c.shape)} on {c.device}")
    return K


# ---------------------------------------------------------------------------------------------------------------- host form
def _tensor(a):
    return torch.from_numpy(np.ascontiguousarray(a)).reshape(np.shape(a))      # (ascontiguousarray makes a 0-dim array 1-dim)


def _clamped(ids, n):
    a = ids.reshape(-1).numpy().astype(np.int64)
    return np.where((a >= 1) & (a <= n), a, 0)


def _table_host(pred, truth, n_p, n_t):
    """``(pairs [P, 2], intersection [P], pred_area, truth_area)`` by a stable sort of the fused keys: a run of equal keys starts at the
    pair's first position, and the runs are put in the order of those."""
    p, t = _clamped(pred, n_p), _clamped(truth, n_t)
    area_p = np.bincount(p, minlength=n_p + 1)[1:].astype(np.int64)
    area_t = np.bincount(t, minlength=n_t + 1)[1:].astype(np.int64)
    both = np.flatnonzero((p > 0) & (t > 0))
    key = (p[both] << 32) | t[both]
    order = np.argsort(key, kind="stable")
    run = key[order]
    start = np.flatnonzero(np.concatenate([[True], run[1:] != run[:-1]])) if run.size else np.zeros(0, np.int64)
    count = np.diff(np.append(start, run.size)).astype(np.int64)
    rows = np.argsort(both[order[start]])
    fused = run[start][rows]
    pairs = np.stack([fused >> 32, fused & 0xFFFFFFFF], axis=1).astype(np.int32).reshape(-1, 2)
    return pairs, count[rows], area_p, area_t


def _scores(tp, fp, fn, sum_iou, over):
    tp_f, half, every = tp.astype(np.float64), tp + fp / 2.0 + fn / 2.0, (tp + fp + fn).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        res = {"sq": np.where(tp > 0, sum_iou / tp_f, np.nan), "rq": np.where(half > 0, tp_f / half, np.nan),
               "pq": np.where(half > 0, sum_iou / half, np.nan), "ap": np.where(every > 0, tp_f / every, np.nan)}
    if over:
        res = {k: np.full_like(v, np.nan) for k, v in res.items()}
    return res


def _match_host(pred, truth, n_p, n_t, m, taus, K, pred_class, truth_class):
    pairs, inter, area_p, area_t = _table_host(pred, truth, n_p, n_t)
    over = len(pairs) > m
    ip, it = pairs[:, 0].astype(np.int64) - 1, pairs[:, 1].astype(np.int64) - 1
    iou = inter.astype(np.float64) / (area_p[ip] + area_t[it] - inter).astype(np.float64)
    ok = iou > taus[0]
    KK = max(K, 1)
    cls_p, cls_t = np.zeros(n_p, np.int64), np.zeros(n_t, np.int64)
    if K:
        cls_p, cls_t = pred_class.numpy().astype(np.int64), truth_class.numpy().astype(np.int64)
        ok &= (cls_p[ip] == cls_t[it]) & (cls_p[ip] >= 0) & (cls_p[ip] < K)
    res = {"pred_match": np.zeros(n_p, np.int32), "truth_match": np.zeros(n_t, np.int32), "pred_iou": np.zeros(n_p), "truth_iou": np.zeros(n_t),
           "pred_area": area_p, "truth_area": area_t}
    res["pred_match"][ip[ok]] = pairs[ok, 1]
    res["truth_match"][it[ok]] = pairs[ok, 0]
    res["pred_iou"][ip[ok]] = iou[ok]
    res["truth_iou"][it[ok]] = iou[ok]
    tp, sum_iou = np.zeros((KK, len(taus)), np.int64), np.zeros((KK, len(taus)))
    present_p, present_t = np.zeros((KK, 1), np.int64), np.zeros((KK, 1), np.int64)
    for k in range(KK):
        present_p[k] = int(((area_p > 0) & (cls_p == k)).sum())
        present_t[k] = int(((area_t > 0) & (cls_t == k)).sum())
        for j, tau in enumerate(taus):
            hit = (res["pred_iou"] > tau) & (cls_p == k)
            tp[k, j] = int(hit.sum())
            sum_iou[k, j] = res["pred_iou"][hit].sum()
    res.update(tp=tp, fp=present_p - tp, fn=present_t - tp, sum_iou=sum_iou)
    res.update(_scores(tp, res["fp"], res["fn"], sum_iou, over))
    res["num_pairs"] = np.array(-1 if over else len(pairs), np.int64)
    return res


# ---------------------------------------------------------------------------------------------------------------- device
def _device(what, pred, truth, n_p, n_t, m, taus, K, pred_class, truth_class):
    """One native call: ``{name: tensor}`` for every output of the plan, views of one zeroed block"""
    dev = pred.device
    T, KK = len(taus), max(K, 1)
    positions = pred.numel()
    slots, ws_bytes, out_bytes = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    offsets = (ctypes.c_int64 * len(_OUTPUTS))()
    rc = N.load().ptb_inst_plan(positions, n_p, n_t, m, T, K, ctypes.byref(slots), ctypes.byref(ws_bytes), offsets, ctypes.byref(out_bytes))
    N.check(rc, what)
    p, t = pred.contiguous(), truth.contiguous()
    out = M.scratch(out_bytes.value, dev)
    ws = M.scratch(ws_bytes.value, dev)
    if T == 0:
        N.launch("ptb_inst_overlaps", dev, p.data_ptr(), t.data_ptr(), positions, n_p, n_t, m, out.data_ptr(), out_bytes.value, ws.data_ptr(),
                 ws_bytes.value, what=what)
    else:
        pc = pred_class.contiguous() if K else None
        tc = truth_class.contiguous() if K else None
        N.launch("ptb_inst_match", dev, p.data_ptr(), t.data_ptr(), positions, n_p, n_t, m, (ctypes.c_double * T)(*taus), T,
                 N.ptr(pc), M.ELEM_BYTES[pc.dtype] if K else 0, N.ptr(tc), M.ELEM_BYTES[tc.dtype] if K else 0, K, out.data_ptr(), out_bytes.value,
                 ws.data_ptr(), ws_bytes.value, what=what)
    rows = m if T == 0 else 0
    shapes = {"num_pairs": (), "pred_area": (n_p,), "truth_area": (n_t,), "pairs": (rows, 2), "intersection": (rows,), "pred_match": (n_p,) if T else (0,),
              "truth_match": (n_t,) if T else (0,), "pred_iou": (n_p,) if T else (0,), "truth_iou": (n_t,) if T else (0,)}
    res = {}
    for name, off in zip(_OUTPUTS, offsets):
        shape = shapes.get(name, (KK, T))
        dtype = torch.int32 if name in _INT32 else torch.float64 if name in _FLOAT64 else torch.int64
        nbytes = math.prod(shape) * (4 if dtype == torch.int32 else 8)
        res[name] = out[off:off + nbytes].view(dtype).reshape(shape)
    return res


def _arguments(what, pred, truth, num_pred, num_truth, max_pairs):
    _maps(what, pred, truth)
    n_p, n_t = _count(what, "num_pred", num_pred, pred), _count(what, "num_truth", num_truth, truth)
    m, given = _pairs_cap(what, max_pairs, pred.numel(), n_p, n_t)
    return n_p, n_t, m, given


# ---------------------------------------------------------------------------------------------------------------- public
def instance_overlaps(pred, truth, num_pred=None, num_truth=None, max_pairs=None):
    """The sparse overlap table of two instance maps: every (pred id, truth id) that occurs at some position, and how often.

    ``pred``, ``truth``: int32 instance maps of the same shape on the same device -- what ``connected_components`` returns, or any map
    whose ids are ``1 .. n`` with 0 as background.  The maps are compared position by position in their flat order, so any shape
    (``[H, W]``, ``[D, H, W]``, anything) is ONE entry: loop over a stack, as with ``component_stats`` (component ids are per entry).  An
    id <= 0 or above that side's ``n`` counts as background on that side.  ``num_pred`` / ``num_truth``: the ``n`` of each side as an int
    (nothing is read back), a 0-dim count tensor (read back, 8 bytes) or ``None`` (``map.max()``, read back).

    Returns a dict: ``"pairs"`` int32 ``[P, 2]``, (pred id, truth id), both >= 1; ``"intersection"`` int64 ``[P]``, the positions that hold
    the pair; ``"pred_area"`` int64 ``[n_pred]`` and ``"truth_area"`` int64 ``[n_truth]``, row ``i`` for id ``i + 1``; ``"num_pairs"`` int64,
    0-dim.  The rows are ordered by the row-major index of the FIRST position at which the pair occurs -- the numbering rule of
    ``connected_components`` applied to pairs --, a function of the input alone.

    ``max_pairs=None``: the table is sized for ``min(positions, num_pred * num_truth, 2^22)`` distinct pairs and ``num_pairs`` is read back
    (8 bytes) to size the rows; more pairs than that raise ``ValueError`` (pass a larger ``max_pairs``).  ``max_pairs=m``: nothing is read
    back, the result has ``m`` rows, rows past the real count are zero, and ``num_pairs == -1`` iff the input has more than ``m`` distinct
    pairs (the other outputs are then unspecified).

    The call is stream-ordered; contiguous CUDA maps are read where they lie, other strides are copied first; the tensors of the
    result are views of one block.  More than 2^31 - 2 positions raise ``ValueError``; empty inputs return without a launch."""
    what = "instance_overlaps"
    n_p, n_t, m, given = _arguments(what, pred, truth, num_pred, num_truth, max_pairs)
    dev = pred.device
    if pred.numel() == 0:
        return {"pairs": torch.zeros((m if given else 0, 2), dtype=torch.int32, device=dev),
                "intersection": torch.zeros(m if given else 0, dtype=torch.int64, device=dev), "pred_area": torch.zeros(n_p, dtype=torch.int64, device=dev),
                "truth_area": torch.zeros(n_t, dtype=torch.int64, device=dev), "num_pairs": torch.zeros((), dtype=torch.int64, device=dev)}
    if not pred.is_cuda:
        pairs, inter, area_p, area_t = _table_host(pred.contiguous(), truth.contiguous(), n_p, n_t)
        P = len(pairs)
        if P > m and not given:
            raise ValueError(f"{what}: more than {m} distinct pairs: pass max_pairs")
        if given:
            rows, cnt = np.zeros((m, 2), np.int32), np.zeros(m, np.int64)
            rows[:min(P, m)], cnt[:min(P, m)] = pairs[:m], inter[:m]
            pairs, inter = rows, cnt
        res = {"pairs": pairs, "intersection": inter, "pred_area": area_p, "truth_area": area_t, "num_pairs": np.array(-1 if P > m else P, np.int64)}
        return {k: _tensor(v) for k, v in res.items()}
    res = _device(what, pred, truth, n_p, n_t, m, (), 0, None, None)
    res = {k: res[k] for k in ("pairs", "intersection", "pred_area", "truth_area", "num_pairs")}
    if not given:
        P = int(res["num_pairs"].item())
        if P < 0:
            raise ValueError(f"{what}: more than {m} distinct pairs: pass max_pairs")
        res["pairs"], res["intersection"] = res["pairs"][:P], res["intersection"][:P]
    return res


def match_instances(pred, truth, thresholds=(0.5,), num_pred=None, num_truth=None, pred_class=None, truth_class=None, num_classes=None, max_pairs=None):
    """The one-to-one matching of the instances of ``pred`` and ``truth`` above IoU 0.5, and the counts and scores per threshold.

    ``pred``, ``truth``, ``num_pred``, ``num_truth``: as in ``instance_overlaps`` (any shape is ONE entry; loop over a stack).
    ``thresholds``: 1 to 16 increasing floats with ``0.5 <= t < 1`` (a float alone is one threshold); below 0.5 a match is no longer unique
    (``ValueError``).  A pair matches at ``t`` iff ``IoU > t``, strictly, with ``IoU = I / (A_p + A_t - I)`` as one float64 division of exact
    integers, and -- when classes are given -- both instances have the same class.  ``pred_class`` / ``truth_class``: integer tensors
    ``[num_pred]`` / ``[num_truth]`` (for example ``component_stats(cc, n, values=labels)["value"]``), given together with
    ``num_classes=K``; an instance whose class is outside ``0 .. K - 1`` never matches and counts nowhere.

    Returns a dict (T thresholds; ``[T]`` becomes ``[K, T]`` with classes): ``"pred_match"`` int32 ``[num_pred]`` and ``"truth_match"`` int32
    ``[num_truth]``, the partner's id at ``thresholds[0]``, 0 if none; ``"pred_iou"`` / ``"truth_iou"`` float64, that partner's IoU, 0 if
    none; ``"pred_area"`` / ``"truth_area"`` int64; ``"tp"``, ``"fp"``, ``"fn"`` int64 ``[T]`` -- a present instance is an id with area > 0,
    ``fp`` = present preds - ``tp``, ``fn`` = present truths - ``tp``; ``"sum_iou"`` float64 ``[T]``, the sum of the matched IoUs;
    ``"sq" = sum_iou / tp``, ``"rq" = tp / (tp + fp / 2 + fn / 2)``, ``"pq" = sum_iou / (tp + fp / 2 + fn / 2)`` (panoptic quality; ``rq`` is
    also the F1 score) and ``"ap" = tp / (tp + fp + fn)`` (the DSB-2018 score per threshold; its mean over thresholds is ``.mean()``),
    float64 ``[T]``, ``nan`` where the denominator is 0; ``"num_pairs"`` int64, 0-dim, the distinct overlapping pairs.

    ``max_pairs``: the table is sized for it (``None``: ``min(positions, num_pred * num_truth, 2^22)``); when the input has more distinct
    pairs, ``num_pairs`` is -1 and every score is ``nan``.  Nothing is read back beyond what ``num_pred`` / ``num_truth`` ask for.  The
    call is stream-ordered and a second run changes no bit, ``sum_iou`` included; the tensors of the result are views of one block.
    Empty inputs return without a launch."""
    what = "match_instances"
    n_p, n_t, m, _ = _arguments(what, pred, truth, num_pred, num_truth, max_pairs)
    taus = _thresholds(what, thresholds)
    dev = pred.device
    K = _classes(what, pred_class, truth_class, num_classes, n_p, n_t, dev)
    T, KK = len(taus), max(K, 1)
    if pred.numel() == 0:
        res = {"pred_match": torch.zeros(n_p, dtype=torch.int32, device=dev), "truth_match": torch.zeros(n_t, dtype=torch.int32, device=dev),
               "pred_iou": torch.zeros(n_p, dtype=torch.float64, device=dev), "truth_iou": torch.zeros(n_t, dtype=torch.float64, device=dev),
               "pred_area": torch.zeros(n_p, dtype=torch.int64, device=dev), "truth_area": torch.zeros(n_t, dtype=torch.int64, device=dev),
               "num_pairs": torch.zeros((), dtype=torch.int64, device=dev)}
        res.update({k: torch.zeros((KK, T), dtype=torch.int64, device=dev) for k in ("tp", "fp", "fn")})
        res["sum_iou"] = torch.zeros((KK, T), dtype=torch.float64, device=dev)
        res.update({k: torch.full((KK, T), math.nan, dtype=torch.float64, device=dev) for k in _SCORES})
    elif not pred.is_cuda:
        host = _match_host(pred.contiguous(), truth.contiguous(), n_p, n_t, m, taus, K, pred_class, truth_class)
        res = {k: _tensor(v) for k, v in host.items()}
    else:
        res = _device(what, pred, truth, n_p, n_t, m, taus, K, pred_class, truth_class)
        del res["pairs"], res["intersection"]
    if not K:
        res.update({k: res[k].reshape(T) for k in _PER_THRESHOLD})
    return res
