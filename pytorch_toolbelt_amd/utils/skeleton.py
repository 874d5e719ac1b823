"""Skeletons of label maps by parallel thinning, and the centreline Dice computed from them, on the device the tensors are on -- the thin
structures of the label-map chain (roads, vessels, neurites, cracks, membranes), which IoU and Hausdorff say little about::

    skel = skeletonize(sem)                                   # the centrelines of everything that is not background
    length = skel.sum((-1, -2))
    score = centerline_dice(pred, truth, labels=[1, 2, 3])    # clDice, tprec, tsens per stack entry and class

The reference has no counterpart, so the names and meanings below are this library's.  CUDA tensors run the HIP kernels of
``csrc/ptb_skeleton.hip`` (a missing kernel is an error, never a silent host computation), CPU tensors take the host form below with the
same bits -- the device the caller names decides.  ``dims=3`` thins volumes ``[*stack, D, H, W]`` (``csrc/ptb_skeleton3d.hip``; definitions further down);
``dims=2``, the default, thins planes, and a 3-D tensor is then a stack of planes.

DEFINITIONS, ``dims=2`` (the published papers are the source; these formulae are the definition).  The neighbours of a position P1 = ``(y, x)``::

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

DEFINITIONS, ``dims=3`` (``method="subfield"``, the only one and the default there; Bertrand & Malandain 1994 for "simple").  Positions are ``(z, y, x)``;
positions outside the entry are background; the object is 26-connected and the background 6-connected; N26(p), N18(p) and N6(p) are the
usual punctured neighbourhoods of p.

* ``p`` is SIMPLE iff the object positions in N26(p) form exactly one 26-connected component, and the background positions in N18(p) that a
  6-path within N18(p) joins to a background member of N6(p) form exactly one 6-connected component (so there is such a member).
* ``p`` is an END POINT iff it has exactly one object position in N26(p).  A position with none is not simple, so it stays.
* The SUBFIELD of p is ``(z & 1) * 4 + (y & 1) * 2 + (x & 1)``, coordinates within the entry.  Two positions of one subfield are never 26-adjacent.
* One ITERATION is six DIRECTION PASSES, in the order ``z-1, z+1, y-1, y+1, x-1, x+1``.  A pass first marks its CANDIDATES from the state at the
  start of the pass: the object positions whose neighbour in the pass's direction is background.  It then runs eight SUB-STEPS, subfield 0 to
  7: sub-step ``f`` deletes every candidate of subfield ``f`` that is still simple and is not an end point in the state before that sub-step.
  (Marking candidates once per pass keeps a pass from peeling two layers.)
* Decisions inside one sub-step cannot see each other, so a sub-step equals deleting simple points one at a time: topology is preserved by
  construction, and the result has no order or tie rule in it.
* Skeleton, iteration count and ``max_iterations`` are as above; the guard of a run to stability is ``D + H + W`` iterations.

Left out: surface skeletons, the template sets of Lee 1994 and of Palagyi, the medial axis with distances (compose it as
``skeletonize(m) * distance_transform(m)``), pruning of spurs and node / branch classification, and ``ignore_index``.  The
soft-clDice training loss is ``losses.SoftClDiceLoss``.
"""
import ctypes

import numpy as np
import torch

from .. import _native as N
from . import _maps as M

__all__ = ["skeletonize", "centerline_dice"]

_METHODS = {"zhang": 0, "guo_hall": 1}          # PTB_THIN_*
_SUBFIELD = "subfield"                          # the method of dims=3
_EQUAL, _NOT_EQUAL = 0, 1                       # PTB_THIN_EQUAL / PTB_THIN_NOT_EQUAL
STEPS = 32                                      # THIN_STEPS of csrc/ptb_skeleton.hip: the sub-iterations of one launch
BRICK, HALO, PASSES = (16, 16, 64), 9, 1         # csrc/ptb_skeleton3d.hip (ptb_thin3d_geometry): the brick of a workgroup (z, y, x), its halo, the direction passes of a launch
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


# the 27-bit cube of a neighbourhood, bit n = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); the 26-bit code leaves the centre's bit 13 out
_U = np.uint32
_CUBE, _X0, _Y0 = 0x7FFFFFF, 0x1249249, 0x7 | 0x7 << 9 | 0x7 << 18
_NOT_X0, _NOT_X2, _NOT_Y0, _NOT_Y2 = (_U(_CUBE & ~m) for m in (_X0, _X0 << 2, _Y0, _Y0 << 6))
_N6 = _U(sum(1 << n for n in (4, 10, 12, 14, 16, 22)))
_N18 = _U(_CUBE & ~sum(1 << n for n in (0, 2, 6, 8, 13, 18, 20, 24, 26)))
_OFFSETS = [(n, n // 9 - 1, n // 3 % 3 - 1, n % 3 - 1) for n in range(27) if n != 13]
_DIRECTIONS = ((1, -1), (1, 1), (2, -1), (2, 1), (3, -1), (3, 1))     # (axis of [B, D, H, W], step) of the six direction passes


def _flood(seed, within, faces_only):
    """the positions of the cubes ``within`` that the positions ``seed`` reach, all codes at once: dilate, mask, until nothing grows"""
    reach = seed
    for _ in range(27):
        x = (reach << _U(1) & _NOT_X0) | (reach >> _U(1) & _NOT_X2)
        if faces_only:
            grown = reach | x | (reach << _U(3) & _NOT_Y0) | (reach >> _U(3) & _NOT_Y2) | reach << _U(9) | reach >> _U(9)
        else:
            grown = reach | x
            grown = grown | (grown << _U(3) & _NOT_Y0) | (grown >> _U(3) & _NOT_Y2)
            grown = grown | grown << _U(9) | grown >> _U(9)
        grown &= within
        if np.array_equal(grown, reach):
            break
        reach = grown
    return reach


def _deletable_host(codes):
    """"simple and not an end point" of the 26-bit codes ``codes`` (uint32): the vectorised twin of thin3d_deletable"""
    obj = (codes & _U(0x1FFF)) | (codes >> _U(13) & _U(0x1FFF)) << _U(14)
    several = (obj & (obj - _U(1))) != 0                                       # none: not simple; one: an end point
    one_object = _flood(obj & (~obj + _U(1)), obj, False) == obj
    bg = _N18 & ~obj
    faces = bg & _N6
    one_background = (faces & ~_flood(faces & (~faces + _U(1)), bg, True)) == 0
    return several & one_object & (faces != 0) & one_background


def _decide(codes, memo):
    """``_deletable_host`` of every code, each distinct code decided once per call of ``_thin3_host``: ``memo`` = [sorted codes, their answers]"""
    u, inverse = np.unique(codes, return_inverse=True)
    at = np.minimum(np.searchsorted(memo[0], u), max(len(memo[0]) - 1, 0))
    known = memo[0][at] == u if len(memo[0]) else np.zeros(u.shape, bool)
    if not known.all():
        new = u[~known]
        allc = np.concatenate([memo[0], new])
        order = np.argsort(allc, kind="stable")
        memo[0], memo[1] = allc[order], np.concatenate([memo[1], _deletable_host(new)])[order]
        at = np.searchsorted(memo[0], u)
    return memo[1][at][inverse.reshape(-1)]


def _thin3_host(s, max_iterations):
    """``(skeleton, iteration count)`` of the bool volumes ``s`` ``[B, D, H, W]``, all thinned together: the docstring's passes and sub-steps, the
    neighbourhood codes of a sub-step's candidates gathered from a zero-padded copy"""
    B, D, H, W = s.shape
    padded = np.zeros((B, D + 2, H + 2, W + 2), bool)
    padded[:, 1:-1, 1:-1, 1:-1] = s
    s = padded[:, 1:-1, 1:-1, 1:-1]
    memo = [np.zeros(0, _U), np.zeros(0, bool)]
    done = 0
    while max_iterations is None or done < max_iterations:
        any_deleted = False
        for axis, step in _DIRECTIONS:
            window = [slice(None), slice(1, D + 1), slice(1, H + 1), slice(1, W + 1)]
            window[axis] = slice(1 + step, 1 + step + s.shape[axis])
            cand = s & ~padded[tuple(window)]
            if not cand.any():
                continue
            for f in range(8):
                sub = (slice(None), slice(f >> 2 & 1, None, 2), slice(f >> 1 & 1, None, 2), slice(f & 1, None, 2))
                b, z, y, x = np.nonzero(cand[sub] & s[sub])
                if not b.size:
                    continue
                z, y, x = 2 * z + (f >> 2 & 1), 2 * y + (f >> 1 & 1), 2 * x + (f & 1)
                codes = np.zeros(b.shape, _U)
                for n, dz, dy, dx in _OFFSETS:
                    codes |= padded[b, z + 1 + dz, y + 1 + dy, x + 1 + dx].astype(_U) << _U(n - (n > 13))
                go = _decide(codes, memo)
                if go.any():
                    any_deleted = True
                    s[b[go], z[go], y[go], x[go]] = False
        if not any_deleted:
            break
        done += 1
    return s.copy(), done


def _object_host(x, rule, value):
    """the object of a label map as a bool array; ``value``: None for one the dtype cannot hold"""
    a = x.numpy()
    eq = np.zeros(a.shape, bool) if value is None else a == (bool(value) if a.dtype == np.bool_ else value)
    return ~eq if rule == _NOT_EQUAL else eq


# ---------------------------------------------------------------------------------------------------------------- public
def _method(what, method, dims):
    """the code of a 2-D method, None for the one of ``dims=3``; ``method=None``: the default of ``dims``"""
    M.check_dims(what, dims)
    if dims == 3:
        if method not in (None, _SUBFIELD):
            raise ValueError(f"{what}: method must be 'subfield' (or None) for dims=3, got {method!r}")
        return None
    if method is None:
        method = "guo_hall"
    if method not in _METHODS:
        raise ValueError(f"{what}: method must be 'guo_hall' or 'zhang', got {method!r}")
    return _METHODS[method]


def _not_converged(what, D, H, W, took, dims):
    guard = f"D + H + W = {D + H + W}" if dims == 3 else f"H + W = {H + W}"
    raise RuntimeError(f"{what}: the thinning did not converge within the guard of {guard} iterations: {int(took[1])} launches run")


def skeletonize(labels, background=0, foreground=None, method=None, max_iterations=None, out=None, return_iterations=False, dims=2):
    """The skeleton of the object of ``labels`` by parallel thinning (the module docstring's definitions), as a ``bool`` tensor of the input's shape.

    ``labels``: ``[*stack, H, W]`` (``dims=3``: ``[*stack, D, H, W]``) of ``bool``, ``uint8``, ``int16``, ``int32`` or ``int64``; the entries of ``stack`` are thinned
    independently, all in the same launches.  The object is, with ``foreground=None``, the positions that do not hold ``background`` and, with ``foreground=c``, the positions that
    hold ``c`` -- ``distance_transform``'s pair of arguments: one class of a multi-class map without making ``labels == c``.  A value the dtype
    cannot hold occurs nowhere.  ``method``: ``"guo_hall"`` (``None`` under ``dims=2``) or ``"zhang"``; under ``dims=3`` ``"subfield"`` (``None``).

    ``max_iterations=None`` runs to stability; ``n >= 0`` stops after at most ``n`` iterations (0 returns the object mask).  ``out``: a ``bool`` or ``uint8``
    tensor of the input's shape and device that receives the result (and is returned); it may be the input.  ``return_iterations=True``:
    also return the iteration count of the call as an int -- that of the entry that took longest.

    CUDA tensors: ONE native call.  Contiguous inputs are read where they lie, packed into bit planes (32 positions a word); other strides
    are copied first.  The thinning kernel runs ``STEPS`` sub-iterations (this module's constant, the library's ``ptb_thin_steps()``) of a
    64 x 64 tile per launch in LDS, only where something still changes; launches go eight at a time on the caller's stream and after each batch one word is read back (and one more at the end, the
    iteration count), so THE CALL SYNCHRONISES ITS STREAM AND CANNOT BE CAPTURED into a graph.  Running to stability is guarded by
    ``H + W`` iterations; a call that gets there raises ``RuntimeError`` (the guard is not a claimed bound: the largest count seen is
    ``min(H, W) / 2``).  The result is a function of the input alone: the same bits on every run.  Bad arguments raise before anything is
    launched; empty inputs return without a launch.

    ``dims=3``: the same call on volumes.  The kernel of ``csrc/ptb_skeleton3d.hip`` holds a brick of ``BRICK`` positions with a halo of ``HALO`` in LDS and
    runs ``PASSES`` direction pass(es) per launch, in place; a brick runs while it or a neighbour changed within the last ``6 / PASSES`` launches.  The
    guard is ``D + H + W`` iterations.  CPU tensors: numpy, the neighbourhood codes of a sub-step's candidates decided once per distinct code."""
    what = "skeletonize"
    M.check_labels(what, "labels", labels)
    code = _method(what, method, dims)
    _, B, D, H, W = M.extent(what, "labels", labels, dims)
    background = M.check_int(what, "background", background, allow_none=True)
    foreground = M.check_int(what, "foreground", foreground, allow_none=True)
    if foreground is None and background is None:
        raise ValueError(f"{what}: background=None needs foreground= (there would be no object)")
    rule, value = (_NOT_EQUAL, background) if foreground is None else (_EQUAL, foreground)
    max_iterations = M.check_int(what, "max_iterations", max_iterations, allow_none=True)
    if max_iterations is not None and max_iterations < 0:
        raise ValueError(f"{what}: max_iterations must be None or >= 0, got {max_iterations}")
    M.check_out(what, out, out.dtype if isinstance(out, torch.Tensor) and out.dtype == torch.uint8 else torch.bool, labels)
    dev = labels.device
    iterations = 0
    if B * D * H * W == 0:
        res = out if out is not None else torch.empty(labels.shape, dtype=torch.bool, device=dev)
    elif not labels.is_cuda:
        obj = _object_host(labels.contiguous().reshape((B, D, H, W) if dims == 3 else (B, H, W)), rule, value if M.fits(value, labels.dtype) else None)
        skel, iterations = _thin3_host(obj, max_iterations) if dims == 3 else _thin_host(obj, code, max_iterations)
        res = torch.from_numpy(skel).reshape(labels.shape)
    else:
        x = labels.contiguous()
        res = out if M.direct_out(out, x) else torch.empty(x.shape, dtype=torch.bool, device=dev)
        took = (ctypes.c_int * 2)(0, 0)
        limit = -1 if max_iterations is None else max_iterations
        if dims == 3:
            ws, nbytes = M.workspace(N.load().ptb_skeleton3d_plan, what, dev, B, D, H, W)
            rc = N.launch("ptb_skeleton3d", dev, x.data_ptr(), M.ELEM_BYTES[x.dtype], B, D, H, W, rule, value, limit, res.data_ptr(), took, ws.data_ptr(), nbytes, raw=True)
        else:
            ws, nbytes = M.workspace(N.load().ptb_skeleton_plan, what, dev, B, H, W)
            rc = N.launch("ptb_skeleton", dev, x.data_ptr(), M.ELEM_BYTES[x.dtype], B, H, W, rule, value, code, limit,
                          res.data_ptr(), took, ws.data_ptr(), nbytes, raw=True)     # (a bool tensor's bytes are the uint8 the kernels write)
        if rc == N.PTB_ENOTCONVERGED:
            _not_converged(what, D, H, W, took, dims)
        N.check(rc, what)
        iterations = int(took[0])
    res = M.finish_out(out, res)
    return (res, iterations) if return_iterations else res


def _plan(what, B, H, W, K, cap, D=1, dims=2):
    """the workspace bytes of a ``centerline_dice`` call; the errors of a shape or a cap that cannot be served"""
    if 2 * K * B * D * H * W > M.MAX_POSITIONS:
        raise ValueError(f"{what}: 2 x {K} x {B * D * H * W} positions (both sides of every class) in one thinning run; at most 2^31 - 2 = {M.MAX_POSITIONS}: split the stack")
    nbytes = ctypes.c_int64()
    lib = N.load()
    N.check(lib.ptb_centerline_dice3d_plan(B, D, H, W, K, ctypes.byref(nbytes)) if dims == 3 else lib.ptb_centerline_dice_plan(B, H, W, K, ctypes.byref(nbytes)), what)
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


def centerline_dice(pred, truth, labels=None, method=None, background=0, max_workspace_bytes=DEFAULT_WORKSPACE_BYTES, dims=2):
    """The centreline Dice (clDice, Shit et al., CVPR 2021) of two label maps ``pred`` and ``truth`` of one shape ``[*stack, H, W]`` (``dims=3``: ``[*stack, D, H, W]``,
    skeletons by 3-D thinning, ``method`` as in ``skeletonize``) on one device, each of a label dtype of its own.  ``labels=None``: one object, the positions that do not hold ``background`` (K = 1).  Otherwise ``labels`` is a sequence of
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
    code = _method(what, method, dims)
    stack, B, D, H, W = M.extent(what, "pred and truth", pred, dims)
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
    if B * D * H * W == 0:
        counts = torch.zeros(stack + (K, 4), dtype=torch.int64, device=dev)
        nan = torch.full(stack + (K,), float("nan"), dtype=torch.float32, device=dev)
        return {"cldice": nan, "tprec": nan.clone(), "tsens": nan.clone(), "counts": counts}
    if not pred.is_cuda:
        entry = (B, D, H, W) if dims == 3 else (B, H, W)
        masks = [np.stack([_object_host(t.contiguous().reshape(entry), rule, v if M.fits(v, t.dtype) else None) for v in values], axis=1) for t in (pred, truth)]
        both = np.stack(masks)                                                  # [2, B, K, (D,) H, W]
        flat = both.reshape((-1,) + entry[1:])
        skel = (_thin3_host(flat, None) if dims == 3 else _thin_host(flat, code, None))[0].reshape(both.shape)
        over = tuple(range(-dims, 0))
        counts = np.stack([(skel[0] & both[1]).sum(over), skel[0].sum(over), (skel[1] & both[0]).sum(over), skel[1].sum(over)], axis=-1).astype(np.int64)
        d, p, s = _ratios(counts)
        res = {"cldice": torch.from_numpy(d), "tprec": torch.from_numpy(p), "tsens": torch.from_numpy(s), "counts": torch.from_numpy(counts)}
    else:
        nbytes = _plan(what, B, H, W, K, cap, D, dims)
        x, y = pred.contiguous(), truth.contiguous()
        ws = M.scratch(nbytes, dev)
        counts = torch.empty((B, K, 4), dtype=torch.int64, device=dev)
        ratios = torch.empty((3, B, K), dtype=torch.float32, device=dev)
        took = (ctypes.c_int * 2)(0, 0)
        tail = (counts.data_ptr(), ratios[0].data_ptr(), ratios[1].data_ptr(), ratios[2].data_ptr(), took, ws.data_ptr(), nbytes)
        if dims == 3:
            rc = N.launch("ptb_centerline_dice3d", dev, x.data_ptr(), M.ELEM_BYTES[x.dtype], y.data_ptr(), M.ELEM_BYTES[y.dtype], B, D, H, W, N.i64_array(values), K, rule,
                          *tail, raw=True)
        else:
            rc = N.launch("ptb_centerline_dice", dev, x.data_ptr(), M.ELEM_BYTES[x.dtype], y.data_ptr(), M.ELEM_BYTES[y.dtype], B, H, W, N.i64_array(values), K, rule,
                          code, *tail, raw=True)
        if rc == N.PTB_ENOTCONVERGED:
            _not_converged(what, D, H, W, took, dims)
        N.check(rc, what)
        res = {"cldice": ratios[0], "tprec": ratios[1], "tsens": ratios[2], "counts": counts}
    return {k: v.reshape(stack + (K, 4) if k == "counts" else stack + (K,)) for k, v in res.items()}
