"""Surface (boundary) metrics of two label maps, on the device the tensors are on: Hausdorff distance, its percentile (HD95), average
symmetric surface distance and surface Dice / normalised surface distance -- the scores that medical and remote-sensing evaluations report
next to the overlap scores of ``segmentation_scores``, from ``merge_crop(argmax=True)`` and the ground truth without leaving the device.

The reference has no counterpart, so the names and meanings below are this library's; the recipe MedPy popularised, written with scipy
alone (``binary_erosion``, ``distance_transform_edt``, ``np.percentile``), is the yardstick.  CUDA tensors run the HIP kernels of
``csrc/ptb_surface.hip`` around ONE ``ptb_edt`` per chunk of classes (a missing kernel is an error, never a silent host computation), CPU
tensors take the numpy form below with the same definitions -- the device the caller names decides.
"""
import ctypes
import itertools
import math

import numpy as np
import torch

from .. import _native as N
from . import _maps as M

__all__ = ["surface_metrics"]

DEFAULT_WORKSPACE_BYTES = 4 << 30        # what this library may hold by default (the size PTB_DEFER_BYTES uses)
MAX_TOLERANCES = 8
_CLASSES, _NOT_BACKGROUND = 0, 1
_KEYS2 = ("directed_hausdorff", "directed_percentile", "mean_surface_distance")
_KEYS1 = ("hausdorff", "hausdorff_percentile", "assd")


# ---------------------------------------------------------------------------------------------------------------- validation
def _floats(what, name, v, lo, hi, most):
    seq = [v] if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_)) else v
    try:
        vals = [float(t) for t in seq]
    except (TypeError, ValueError):
        raise TypeError(f"{what}: {name} must be a float{'' if most == 1 else f' or a sequence of 1 to {most} floats'}, got {v!r}") from None
    if not 1 <= len(vals) <= most:
        raise ValueError(f"{what}: {name} must have 1 to {most} entries, got {len(vals)}")
    if not all(lo <= t <= hi for t in vals):               # (nan fails both comparisons)
        raise ValueError(f"{what}: {name} must lie in [{lo:g}, {hi:g}], got {vals}")
    return vals


def _arguments(what, pred, truth, labels, background, dims, spacing, connectivity, percentile, tolerance, max_workspace_bytes):
    for name, t in (("pred", pred), ("truth", truth)):
        M.check_labels(what, name, t)
    M.check_dims(what, dims)
    if pred.shape != truth.shape:
        raise ValueError(f"{what}: pred and truth must have the same shape, got {tuple(pred.shape)} and {tuple(truth.shape)}")
    if pred.device != truth.device:
        raise ValueError(f"{what}: pred and truth must be on the same device, got {pred.device} and {truth.device}")
    stack, B, D, H, W = M.extent(what, "pred and truth", pred, dims, squares=True)
    connectivity, full = M.check_connectivity(what, connectivity, dims, default=0)
    if labels is None:
        values, rule = [M.check_int(what, "background", background)], _NOT_BACKGROUND
    else:
        try:
            values = list(labels)
        except TypeError:
            raise TypeError(f"{what}: labels must be None or a sequence of class values, got {labels!r}") from None
        if not values:
            raise ValueError(f"{what}: labels must name at least one class")
        values, rule = [M.check_int(what, "labels", v) for v in values], _CLASSES
    sp = M.spacing(what, spacing, dims)
    pct = _floats(what, "percentile", percentile, 0.0, 100.0, 1)[0]
    tols = _floats(what, "tolerance", tolerance, 0.0, math.inf, MAX_TOLERANCES)
    if max_workspace_bytes is None:
        cap = DEFAULT_WORKSPACE_BYTES
    else:
        cap = M.check_int(what, "max_workspace_bytes", max_workspace_bytes)
        if cap < 1:
            raise ValueError(f"{what}: max_workspace_bytes must be positive, got {cap}")
    return stack, B, D, H, W, connectivity, full, values, rule, sp, pct, tols, cap


def _plan(what, lib, dims, B, D, H, W, K, cap):
    """``(classes per chunk, workspace bytes, bytes of the one-class minimum)`` of a call; the errors of a shape or a cap that cannot be served"""
    chunk, slots = ctypes.c_int(), ctypes.c_int()
    nbytes, least = ctypes.c_int64(), ctypes.c_int64(-1)
    rc = lib.ptb_surface_plan(dims, B, D, H, W, K, cap, ctypes.byref(chunk), ctypes.byref(nbytes), ctypes.byref(least), ctypes.byref(slots))
    if rc == N.PTB_EUNSUPPORTED:
        raise ValueError(f"{what}: 2 x {B * D * H * W} positions (the two border maps of one class) in one transform; at most 2^31 - 2: split the stack")
    if rc != 0 and least.value >= 0:
        raise ValueError(f"{what}: max_workspace_bytes={cap} is below the {least.value} bytes that one class at a time needs")
    N.check(rc, what)
    return chunk.value, nbytes.value, least.value


def _workspace_plan(shape, classes=1, dims=2, max_workspace_bytes=None):
    """``dict(chunk=, bytes=, minimum=)``: how a call on maps of ``shape`` with ``classes`` classes is chunked under ``max_workspace_bytes``, the
    workspace it allocates and the smallest cap that is accepted (one class per chunk).  Not part of the interface: the tests and
    tools/bench_surface.py ask it what ``surface_metrics`` will do; the arguments are checked as that function checks its own."""
    what = "surface_metrics"
    probe = torch.empty(tuple(M.check_int(what, "shape", s) for s in shape), dtype=torch.uint8, device="meta")
    classes = M.check_int(what, "classes", classes)
    if classes < 1:
        raise ValueError(f"{what}: classes must be positive, got {classes}")
    _, B, D, H, W, *_, cap = _arguments(what, probe, probe, None, 0, dims, None, None, 95.0, 1.0, max_workspace_bytes)
    if B * D * H * W == 0:
        raise ValueError(f"{what}: empty maps of shape {tuple(probe.shape)} take no workspace")
    chunk, nbytes, least = _plan(what, N.load(), dims, B, D, H, W, classes, cap)
    return dict(chunk=chunk, bytes=nbytes, minimum=least)


# ---------------------------------------------------------------------------------------------------------------- host form
def _shifts(dims, full):
    """the offsets (dz, dy, dx) of the neighbours of a position: those that share a face, with ``full`` also an edge or a corner"""
    out = []
    for off in itertools.product((-1, 0, 1), repeat=dims):
        n = sum(abs(o) for o in off)
        if n and (full or n == 1):
            out.append((0,) * (3 - dims) + off)
    return out


def _border_host(a, shifts):
    """the positions of ``a`` (bool [D, H, W]) with a neighbour that is not in ``a`` or lies outside the map"""
    padded = np.zeros(tuple(s + 2 for s in a.shape), bool)
    padded[1:-1, 1:-1, 1:-1] = a
    inner = a.copy()
    D, H, W = a.shape
    for dz, dy, dx in shifts:
        inner &= padded[1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    return a & ~inner


def _percentile_host(s, q):
    """``np.percentile``'s linear rule on the sorted float64 ``s``; an infinite statistic stays infinite, a weight of 0 takes the lower one as it is"""
    if not len(s):
        return np.nan
    pos = (len(s) - 1) * q
    lo = int(math.floor(pos))
    w = pos - lo
    if w == 0.0 or np.isinf(s[lo]):
        return s[lo]
    return s[lo] + (s[lo + 1] - s[lo]) * w


def _host(pred, truth, B, D, H, W, dims, full, values, rule, sp, pct, tols):
    K, T = len(values), len(tols)
    p, t = pred.reshape(B, D, H, W).numpy(), truth.reshape(B, D, H, W).numpy()
    shifts = _shifts(dims, full)
    res = {"surface_count": np.zeros((B, K, 2), np.int64), "surface_dice": np.full((B, K, T), np.nan, np.float32)}
    for key in _KEYS2:
        res[key] = np.full((B, K, 2), np.nan, np.float32)
    for key in _KEYS1:
        res[key] = np.full((B, K), np.nan, np.float32)

    def member(a, dtype, v):
        if rule == _CLASSES:
            return (a == v) if M.fits(v, dtype) else np.zeros(a.shape, bool)
        return (a != v) if M.fits(v, dtype) else np.ones(a.shape, bool)

    q = pct / 100.0
    for b in range(B):
        for k, v in enumerate(values):
            border = np.stack([_border_host(member(p[b], pred.dtype, v), shifts), _border_host(member(t[b], truth.dtype, v), shifts)])
            sq = M.edt_host(border, sp)[0]                                   # [2, D, H, W]: squared distances to pred's, truth's surface
            n = border.reshape(2, -1).sum(axis=1)
            res["surface_count"][b, k] = n
            sets, within = [], np.zeros(T, np.int64)
            for side in range(2):
                key = sq[1 - side][border[side]]
                if sp is None:
                    d = np.where(key >= M.HOST_INF, np.inf, np.sqrt(np.minimum(key, M.HOST_INF - 1).astype(np.float64)))
                    for i, tol in enumerate(tols):
                        within[i] += int((key <= math.floor(min(tol * tol, float(M.INT_INF - 1)))).sum())
                else:
                    d = np.sqrt(key)
                    for i, tol in enumerate(tols):
                        within[i] += int((key.astype(np.float32) <= min(np.float32(tol * tol), np.finfo(np.float32).max)).sum())
                d = np.sort(d)
                sets.append(d)
                if n[side]:
                    res["directed_hausdorff"][b, k, side] = d[-1]
                    res["directed_percentile"][b, k, side] = _percentile_host(d, q)
                    res["mean_surface_distance"][b, k, side] = d.mean() if np.isfinite(d[-1]) else np.inf
            if not n.any():
                continue
            res["surface_dice"][b, k] = within / float(n.sum())
            res["hausdorff_percentile"][b, k] = _percentile_host(np.sort(np.concatenate(sets)), q)
            if n.all():
                res["hausdorff"][b, k] = max(sets[0][-1], sets[1][-1])
                res["assd"][b, k] = (sets[0].mean() + sets[1].mean()) * 0.5
            else:
                res["hausdorff"][b, k] = res["assd"][b, k] = np.inf
    return {key: torch.from_numpy(v) for key, v in res.items()}


# ---------------------------------------------------------------------------------------------------------------- public
def surface_metrics(pred, truth, labels=None, *, background=0, dims=2, spacing=None, connectivity=None, percentile=95.0, tolerance=1.0,
                    max_workspace_bytes=None):
    """Hausdorff distance, its percentile, mean surface distances and surface Dice of the objects of ``pred`` against those of ``truth``.

    ``pred``, ``truth``: integer label maps (``bool``, ``uint8``, ``int16``, ``int32``, ``int64``; each its own dtype) of equal shape
    ``[*stack, H, W]`` (``dims=2``) or ``[*stack, D, H, W]`` (``dims=3``) on the same device; the entries of ``stack`` are scored
    independently, all in the same launches.  ``labels=None``: one object, the positions that do not hold ``background``.  Otherwise a
    sequence of K >= 1 class values; object k is the set of positions that hold ``labels[k]``.  A value the dtype cannot hold occurs nowhere.

    The SURFACE of an object A: the positions of A with at least one ``connectivity``-neighbour (4 or 8 for ``dims=2``, 6 or 26 for ``dims=3``,
    numbered as in ``connected_components``; ``None``: 4 / 6) that is not in A or lies outside the map --
    ``A ^ scipy.ndimage.binary_erosion(A, generate_binary_structure(dims, 1 or dims))``.  The directed sample set ``pred -> truth``: the
    Euclidean distance (``spacing`` as in ``distance_transform``) from every surface position of pred's object to the nearest surface
    position of truth's object; ``truth -> pred`` is the mirror.

    Returns a dict of tensors on the inputs' device (K = 1 with ``labels=None``, T = number of tolerances):

    ``"surface_count"``          ``[*stack, K, 2]`` int64    number of surface positions (pred, truth)
    ``"directed_hausdorff"``     ``[*stack, K, 2]`` float32  maximum of each directed set (``pred -> truth``, ``truth -> pred``)
    ``"hausdorff"``              ``[*stack, K]``             the larger of the two
    ``"directed_percentile"``    ``[*stack, K, 2]``          ``np.percentile(set, percentile)``: linear interpolation between the order statistics
                                                             at ``(n - 1) * percentile / 100``
    ``"hausdorff_percentile"``   ``[*stack, K]``             the same percentile of the two sets POOLED (MedPy's ``hd95``).  The other common
                                                             convention, the larger of the two directed percentiles, is
                                                             ``directed_percentile.amax(-1)``
    ``"mean_surface_distance"``  ``[*stack, K, 2]``          mean of each directed set
    ``"assd"``                   ``[*stack, K]``             mean of the two means
    ``"surface_dice"``           ``[*stack, K, T]``          (samples <= tolerance in both sets) / (sizes of both sets), per entry of ``tolerance``
                                                             (a float or 1 to 8 floats >= 0)

    EMPTY SURFACES.  A direction without samples gives ``nan`` in the directed results.  Both surfaces empty: ``nan`` in every symmetric
    result and in ``surface_dice``.  Exactly one empty: ``inf`` in ``hausdorff``, ``hausdorff_percentile`` and ``assd`` and 0 in
    ``surface_dice`` (the other side samples the ``inf`` that ``distance_transform`` documents for an entry without a site).

    The classes are worked off in chunks that share one distance transform each -- 2 x chunk x stack maps per launch; the workspace (17
    bytes per position of those maps) stays within ``max_workspace_bytes`` (default 4 GiB).  One class at a time is the least: a cap below
    that, or a stack whose two border maps pass 2^31 - 2 positions, raises ``ValueError``.  The chunking changes no bit of any result, and
    neither does a second run.  The call is stream-ordered and reads nothing back; contiguous CUDA inputs are read where they lie (no
    ``labels == c``, widened or boolean copy).  Empty inputs return without a launch."""
    what = "surface_metrics"
    stack, B, D, H, W, connectivity, full, values, rule, sp, pct, tols, cap = _arguments(what, pred, truth, labels, background, dims, spacing, connectivity,
                                                                                         percentile, tolerance, max_workspace_bytes)
    K, T = len(values), len(tols)
    dev = pred.device
    if B * D * H * W == 0:
        res = {"surface_count": torch.zeros((B, K, 2), dtype=torch.int64, device=dev), "surface_dice": torch.full((B, K, T), math.nan, device=dev)}
        res.update({key: torch.full((B, K, 2), math.nan, device=dev) for key in _KEYS2})
        res.update({key: torch.full((B, K), math.nan, device=dev) for key in _KEYS1})
    elif not pred.is_cuda:
        res = _host(pred.contiguous(), truth.contiguous(), B, D, H, W, dims, full, values, rule, sp, pct, tols)
    else:
        _, nbytes, _ = _plan(what, N.load(), dims, B, D, H, W, K, cap)
        p, t = pred.contiguous(), truth.contiguous()
        res = {"surface_count": torch.empty((B, K, 2), dtype=torch.int64, device=dev), "surface_dice": torch.empty((B, K, T), dtype=torch.float32, device=dev)}
        res.update({key: torch.empty((B, K, 2), dtype=torch.float32, device=dev) for key in _KEYS2})
        res.update({key: torch.empty((B, K), dtype=torch.float32, device=dev) for key in _KEYS1})
        ws = M.scratch(nbytes, dev)
        N.launch("ptb_surface_metrics", dev, p.data_ptr(), M.ELEM_BYTES[p.dtype], t.data_ptr(), M.ELEM_BYTES[t.dtype], dims, B, D, H, W,
                 N.i64_array(values), K, rule, connectivity, (ctypes.c_double * 3)(*sp) if sp is not None else None, pct, (ctypes.c_double * T)(*tols), T,
                 res["surface_count"].data_ptr(), res["directed_hausdorff"].data_ptr(), res["hausdorff"].data_ptr(),
                 res["directed_percentile"].data_ptr(), res["hausdorff_percentile"].data_ptr(),
                 res["mean_surface_distance"].data_ptr(), res["assd"].data_ptr(), res["surface_dice"].data_ptr(), ws.data_ptr(), nbytes, what=what)
    return {key: v.reshape(stack + tuple(v.shape[1:])) for key, v in res.items()}
