"""Skeletons of label maps by parallel thinning, and the centreline Dice computed from them, on the device the tensors are on -- the thin
structures of the label-map chain (roads, vessels, neurites, cracks, membranes), which IoU and Hausdorff say little about::

    skel = skeletonize(sem)                                   # the centrelines of everything that is not background
    length = skel.sum((-1, -2))
    score = centerline_dice(pred, truth, labels=[1, 2, 3])    # clDice, tprec, tsens per stack entry and class

The reference has no counterpart, so the names and meanings below are this library's.  CUDA tensors run the HIP kernels of
``csrc/ptb_skeleton.hip`` (a missing kernel is an error, never a silent host computation), CPU tensors take the host form below with the
same bits -- the device the caller names decides.

DEFINITIONS (the published papers are the source; these formulae are the definition).  The neighbours of a position P1 = ``(y, x)``::

    P9 (y-1, x-1)   P2 (y-1, x)   P3 (y-1, x+1)
    P8 (y,   x-1)   P1            P4 (y,   x+1)
    P7 (y+1, x-1)   P6 (y+1, x)   P5 (y+1, x+1)

Positions outside the entry are background.  One ITERATION is sub-iteration 0 followed by sub-iteration 1.  Each sub-iteration is
SYNCHRONOUS: every decision reads the state from before that sub-iteration.  An object position is deleted in sub-iteration ``k`` iff

``method="zhang"`` (Zhang & Suen 1984): with ``B`` the number of set neighbours and ``A`` the number of ``i`` with ``P_i = 0`` and ``P_i+1 = 1`` in the cycle
P2, P3, ..., P9, P2: ``2 <= B <= 6`` and ``A == 1`` and, for ``k = 0``, ``P2 P4 P6 == 0`` and ``P4 P6 P8 == 0``; for ``k = 1``, ``P2 P4 P8 == 0`` and ``P2 P6 P8 == 0``.

``method="guo_hall"`` (Guo & Hall 1989, as in OpenCV's ``ximgproc.thinning``; the default): with
``C = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))``, ``N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8)``,
``N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9)``, ``N = min(N1, N2)`` and ``m = (P6|P7|!P9) & P8`` for ``k = 0``, ``m = (P2|P3|!P5) & P4`` for ``k = 1``:
``C == 1`` and ``2 <= N <= 3`` and ``m == 0``.

THE SKELETON is the state after the first iteration that deletes nothing; with ``max_iterations=n`` the state after at most ``n`` iterations
(``n = 0``: the object mask).  THE ITERATION COUNT is the number of iterations that deleted something.  ``zhang`` deletes a 2 x 2 square
entirely (and so can lose a component); ``guo_hall`` keeps one position of it.

Left out: 3-D thinning (Lee 1994 / Palagyi; there is no ``dims`` argument yet), the medial axis with distances (compose it as
``skeletonize(m) * distance_transform(m)``), pruning of spurs and node / branch classification, ``ignore_index``, and the soft-clDice
training loss with its gradients.
"""
import ctypes

import numpy as np
import torch

from .. import _native as N
from . import _maps as M

__all__ = ["skeletonize", "centerline_dice"]

_METHODS = {"zhang": 0, "guo_hall": 1}          # PTB_THIN_*
_EQUAL, _NOT_EQUAL = 0, 1                       # PTB_THIN_EQUAL / PTB_THIN_NOT_EQUAL
STEPS = 32                                      # THIN_STEPS of csrc/ptb_skeleton.hip: the sub-iterations of one launch
MAX_CLASSES = 32
DEFAULT_WORKSPACE_BYTES = 4 << 30


# ---------------------------------------------------------------------------------------------------------------- host form
def _deleted(s, method, k):
    """the positions of ``s`` (bool ``[B, H, W]``) that sub-iteration ``k`` deletes: shifted views of the padded map and the formulae of the docstring"""
    H, W = s.shape[1:]
    p = np.pad(s, ((0, 0), (1, 1), (1, 1)))
    P2, P3, P4, P5, P6, P7, P8, P9 = (p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in
                                      ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1)))

    def count(terms):
        return sum(t.astype(np.uint8) for t in terms)

    if method == _METHODS["zhang"]:
        ring = (P2, P3, P4, P5, P6, P7, P8, P9)
        b = count(ring)
        a = count(~ring[i] & ring[(i + 1) % 8] for i in range(8))
        side = ~(P2 & P4 & P6) & ~(P4 & P6 & P8) if k == 0 else ~(P2 & P4 & P8) & ~(P2 & P6 & P8)
        return s & (b >= 2) & (b <= 6) & (a == 1) & side
    c = count((~P2 & (P3 | P4), ~P4 & (P5 | P6), ~P6 & (P7 | P8), ~P8 & (P9 | P2)))
    n = np.minimum(count((P9 | P2, P3 | P4, P5 | P6, P7 | P8)), count((P2 | P3, P4 | P5, P6 | P7, P8 | P9)))
    m = (P6 | P7 | ~P9) & P8 if k == 0 else (P2 | P3 | ~P5) & P4
    return s & (c == 1) & (n >= 2) & (n <= 3) & ~m


def _thin_host(s, method, max_iterations):
    """``(skeleton, iteration count)`` of the bool maps ``s`` ``[B, H, W]``, all thinned together"""
    s = s.copy()
    done = 0
    while max_iterations is None or done < max_iterations:
        any_deleted = False
        for k in (0, 1):
            d = _deleted(s, method, k)
            if d.any():
                any_deleted = True
                s &= ~d
        if not any_deleted:
            break
        done += 1
    return s, done


def _object_host(x, rule, value):
    """the object of a label map as a bool array; ``value``: None for one the dtype cannot hold"""
    a = x.numpy()
    eq = np.zeros(a.shape, bool) if value is None else a == (bool(value) if a.dtype == np.bool_ else value)
    return ~eq if rule == _NOT_EQUAL else eq


# ---------------------------------------------------------------------------------------------------------------- public
def _method(what, method):
    if method not in _METHODS:
        raise ValueError(f"{what}: method must be 'guo_hall' or 'zhang', got {method!r}")
    return _METHODS[method]


def _not_converged(what, H, W, took):
    raise RuntimeError(f"{what}: the thinning did not converge within the guard of H + W = {H + W} iterations: {int(took[1])} launches run")


def skeletonize(labels, background=0, foreground=None, method="guo_hall", max_iterations=None, out=None, return_iterations=False):
    """The skeleton of the object of ``labels`` by parallel thinning (the module docstring's definitions), as a ``bool`` tensor of the input's shape.

    ``labels``: ``[*stack, H, W]`` of ``bool``, ``uint8``, ``int16``, ``int32`` or ``int64``; the entries of ``stack`` are thinned independently, all in the same
    launches.  The object is, with ``foreground=None``, the positions that do not hold ``background`` and, with ``foreground=c``, the positions that
    hold ``c`` -- ``distance_transform``'s pair of arguments: one class of a multi-class map without making ``labels == c``.  A value the dtype
    cannot hold occurs nowhere.  ``method``: ``"guo_hall"`` or ``"zhang"``.

    ``max_iterations=None`` runs to stability; ``n >= 0`` stops after at most ``n`` iterations (0 returns the object mask).  ``out``: a ``bool`` or ``uint8``
    tensor of the input's shape and device that receives the result (and is returned); it may be the input.  ``return_iterations=True``:
    also return the iteration count of the call as an int -- that of the entry that took longest.

    CUDA tensors: ONE native call.  Contiguous inputs are read where they lie, packed into bit planes (32 positions a word); other strides
    are copied first.  The thinning kernel runs ``STEPS`` sub-iterations (this module's constant, the library's ``ptb_thin_steps()``) of a
    64 x 64 tile per launch in LDS, only where something still changes; launches go eight at a time on the caller's stream and after each batch one word is read back (and one more at the end, the
    iteration count), so THE CALL SYNCHRONISES ITS STREAM AND CANNOT BE CAPTURED into a graph.  Running to stability is guarded by
    ``H + W`` iterations; a call that gets there raises ``RuntimeError`` (the guard is not a claimed bound: the largest count seen is
    ``min(H, W) / 2``).  The result is a function of the input alone: the same bits on every run.  Bad arguments raise before anything is
    launched; empty inputs return without a launch."""
    what = "skeletonize"
    M.check_labels(what, "labels", labels)
    _, B, _, H, W = M.extent(what, "labels", labels, 2)
    background = M.check_int(what, "background", background, allow_none=True)
    foreground = M.check_int(what, "foreground", foreground, allow_none=True)
    if foreground is None and background is None:
        raise ValueError(f"{what}: background=None needs foreground= (there would be no object)")
    rule, value = (_NOT_EQUAL, background) if foreground is None else (_EQUAL, foreground)
    code = _method(what, method)
    max_iterations = M.check_int(what, "max_iterations", max_iterations, allow_none=True)
    if max_iterations is not None and max_iterations < 0:
        raise ValueError(f"{what}: max_iterations must be None or >= 0, got {max_iterations}")
    M.check_out(what, out, out.dtype if isinstance(out, torch.Tensor) and out.dtype == torch.uint8 else torch.bool, labels)
    dev = labels.device
    iterations = 0
    if B * H * W == 0:
        res = out if out is not None else torch.empty(labels.shape, dtype=torch.bool, device=dev)
    elif not labels.is_cuda:
        obj = _object_host(labels.contiguous().reshape(B, H, W), rule, value if M.fits(value, labels.dtype) else None)
        skel, iterations = _thin_host(obj, code, max_iterations)
        res = torch.from_numpy(skel).reshape(labels.shape)
    else:
        x = labels.contiguous()
        res = out if M.direct_out(out, x) else torch.empty(x.shape, dtype=torch.bool, device=dev)
        ws, nbytes = M.workspace(N.load().ptb_skeleton_plan, what, dev, B, H, W)
        took = (ctypes.c_int * 2)(0, 0)
        rc = N.launch("ptb_skeleton", dev, x.data_ptr(), M.ELEM_BYTES[x.dtype], B, H, W, rule, value, code, -1 if max_iterations is None else max_iterations,
                      res.data_ptr(), took, ws.data_ptr(), nbytes, raw=True)     # (a bool tensor's bytes are the uint8 the kernels write)
        if rc == N.PTB_ENOTCONVERGED:
            _not_converged(what, H, W, took)
        N.check(rc, what)
        iterations = int(took[0])
    res = M.finish_out(out, res)
    return (res, iterations) if return_iterations else res


def _plan(what, B, H, W, K, cap):
    """the workspace bytes of a ``centerline_dice`` call; the errors of a shape or a cap that cannot be served"""
    if 2 * K * B * H * W > M.MAX_POSITIONS:
        raise ValueError(f"{what}: 2 x {K} x {B * H * W} positions (both sides of every class) in one thinning run; at most 2^31 - 2 = {M.MAX_POSITIONS}: split the stack")
    nbytes = ctypes.c_int64()
    N.check(N.load().ptb_centerline_dice_plan(B, H, W, K, ctypes.byref(nbytes)), what)
    if nbytes.value > cap:
        raise ValueError(f"{what}: the call needs a workspace of {nbytes.value} bytes, above max_workspace_bytes={cap}")
    return nbytes.value


def _ratios(counts):
    """``(cldice, tprec, tsens)`` as float32 from int64 counts ``[..., 4]``: float64 in the documented order, rounded once"""
    c = counts.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = np.where(counts[..., 1] != 0, c[..., 0] / c[..., 1], np.nan)
        s = np.where(counts[..., 3] != 0, c[..., 2] / c[..., 3], np.nan)
        d = 2.0 * p * s / (p + s)
    one_empty = (counts[..., 1] == 0) != (counts[..., 3] == 0)
    d = np.where(one_empty | (p + s == 0.0), 0.0, d)
    d = np.where((counts[..., 1] == 0) & (counts[..., 3] == 0), np.nan, d)
    return d.astype(np.float32), p.astype(np.float32), s.astype(np.float32)


def centerline_dice(pred, truth, labels=None, method="guo_hall", background=0, max_workspace_bytes=DEFAULT_WORKSPACE_BYTES):
    """The centreline Dice (clDice, Shit et al., CVPR 2021) of two label maps ``pred`` and ``truth`` of one shape ``[*stack, H, W]`` on one device, each of a
    label dtype of its own.  ``labels=None``: one object, the positions that do not hold ``background`` (K = 1).  Otherwise ``labels`` is a sequence of
    at most 32 class values.  With ``S`` the skeleton (``method``, run to stability) and ``V`` the mask of a class in each map::

        tprec = |S_P & V_T| / |S_P|        tsens = |S_T & V_P| / |S_T|        cldice = 2 tprec tsens / (tprec + tsens)

    Returns a dict of tensors on the inputs' device: ``"cldice"``, ``"tprec"``, ``"tsens"`` float32 ``[*stack, K]`` and ``"counts"`` int64 ``[*stack, K, 4]`` holding
    ``|S_P & V_T|``, ``|S_P|``, ``|S_T & V_P|``, ``|S_T|``.  The counts are exact; the ratios are evaluated in float64 in exactly that order and rounded once to
    float32.  An empty skeleton gives ``nan`` for its own ratio; ``cldice`` is ``nan`` when both skeletons are empty and 0 when exactly one is, or when
    ``tprec + tsens == 0``.

    CUDA tensors: ONE native call, one thinning run over the ``2 K`` bit planes of every stack entry, then popcounts and integer atomics
    (order-free: the same bits on every run).  Nothing is read back but the thinning loop's words, so, like ``skeletonize``, THE CALL
    SYNCHRONISES ITS STREAM AND CANNOT BE CAPTURED into a graph.  The workspace is three bit planes per side and class; a call that would
    need more than ``max_workspace_bytes`` (default 4 GiB) raises ``ValueError`` and says how many bytes it needs -- nothing is chunked."""
    what = "centerline_dice"
    for name, t in (("pred", pred), ("truth", truth)):
        M.check_labels(what, name, t)
    if pred.shape != truth.shape:
        raise ValueError(f"{what}: pred and truth must have the same shape, got {tuple(pred.shape)} and {tuple(truth.shape)}")
    if pred.device != truth.device:
        raise ValueError(f"{what}: pred and truth must be on the same device, got {pred.device} and {truth.device}")
    stack, B, _, H, W = M.extent(what, "pred and truth", pred, 2)
    code = _method(what, method)
    if labels is None:
        values, rule = [M.check_int(what, "background", background)], _NOT_EQUAL
    else:
        try:
            values = list(labels)
        except TypeError:
            raise TypeError(f"{what}: labels must be None or a sequence of class values, got {labels!r}") from None
        if not 1 <= len(values) <= MAX_CLASSES:
            raise ValueError(f"{what}: labels must name between 1 and {MAX_CLASSES} classes, got {len(values)}")
        values, rule = [M.check_int(what, "labels", int(v) if isinstance(v, torch.Tensor) else v) for v in values], _EQUAL
    K = len(values)
    cap = M.check_int(what, "max_workspace_bytes", max_workspace_bytes)
    if cap < 1:
        raise ValueError(f"{what}: max_workspace_bytes must be positive, got {cap}")
    dev = pred.device
    if B * H * W == 0:
        counts = torch.zeros(stack + (K, 4), dtype=torch.int64, device=dev)
        nan = torch.full(stack + (K,), float("nan"), dtype=torch.float32, device=dev)
        return {"cldice": nan, "tprec": nan.clone(), "tsens": nan.clone(), "counts": counts}
    if not pred.is_cuda:
        masks = [np.stack([_object_host(t.contiguous().reshape(B, H, W), rule, v if M.fits(v, t.dtype) else None) for v in values], axis=1) for t in (pred, truth)]
        both = np.stack(masks)                                                  # [2, B, K, H, W]
        skel = _thin_host(both.reshape(-1, H, W), code, None)[0].reshape(both.shape)
        counts = np.stack([(skel[0] & both[1]).sum((-1, -2)), skel[0].sum((-1, -2)), (skel[1] & both[0]).sum((-1, -2)), skel[1].sum((-1, -2))], axis=-1).astype(np.int64)
        d, p, s = _ratios(counts)
        res = {"cldice": torch.from_numpy(d), "tprec": torch.from_numpy(p), "tsens": torch.from_numpy(s), "counts": torch.from_numpy(counts)}
    else:
        nbytes = _plan(what, B, H, W, K, cap)
        x, y = pred.contiguous(), truth.contiguous()
        ws = M.scratch(nbytes, dev)
        counts = torch.empty((B, K, 4), dtype=torch.int64, device=dev)
        ratios = torch.empty((3, B, K), dtype=torch.float32, device=dev)
        took = (ctypes.c_int * 2)(0, 0)
        rc = N.launch("ptb_centerline_dice", dev, x.data_ptr(), M.ELEM_BYTES[x.dtype], y.data_ptr(), M.ELEM_BYTES[y.dtype], B, H, W, N.i64_array(values), K, rule,
                      code, counts.data_ptr(), ratios[0].data_ptr(), ratios[1].data_ptr(), ratios[2].data_ptr(), took, ws.data_ptr(), nbytes, raw=True)
        if rc == N.PTB_ENOTCONVERGED:
            _not_converged(what, H, W, took)
        N.check(rc, what)
        res = {"cldice": ratios[0], "tprec": ratios[1], "tsens": ratios[2], "counts": counts}
    return {k: v.reshape(stack + (K, 4) if k == "counts" else stack + (K,)) for k, v in res.items()}
