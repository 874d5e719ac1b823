"""Marker-controlled watershed, on the device the tensors are on: the step that splits touching objects by FLOODING a landscape -- the
negated distance map, or a model's boundary / centre probability -- from one core per object::

    cores, n = connected_components(distance_transform(sem) > r)           # one core per object
    inst = watershed(-distance_transform(sem), cores, mask=sem != 0)       # every object pixel joins the core whose flood reaches it

``expand_labels`` answers the easier, Euclidean question and lets a label cross a gap; the flood stays inside the mask and follows
the landscape.  The reference has no counterpart, so the names and meanings below are this library's.  CUDA tensors run the HIP kernels
of ``csrc/ptb_watershed.hip`` (a missing kernel is an error, never a silent host computation), CPU tensors take the heap flood below
with the same results, ties included -- the device the caller names decides.

THE DEFINITION.  A sequential priority flood decides ties by the order of its queue; this one is order-free.  Per stack entry, with
``M`` the flooded set (``mask`` non-zero, ``height`` neither NaN nor ``+inf``), the seeds ``S`` the positions of ``M`` whose marker is not
``background``, and paths running over neighbouring positions of ``M``:

1. ``C(p)``, the PASS HEIGHT: the minimum over paths from a seed to ``p`` of the maximum height on the path, ends included (``+inf`` without
   a path) -- the landscape with minima imposed at the markers.
2. A step ``q -> p`` is ADMISSIBLE iff ``C(q) <= C(p)``: the steps a flood can take.  ``D(p)``: the fewest admissible steps from a seed to ``p``.
3. ``sigma(p)``: the smallest linear index ``(z * H + y) * W + x`` among the seeds with an admissible path of exactly ``D(p)`` steps to ``p``.

The result is ``markers[sigma(p)]``.  Where exactly one marker label attains ``C(p)`` every flooding watershed gives that label, and so
does this one; on ties other implementations' answers depend on their queues and are not comparable bit for bit.

Left out: watershed lines, compactness, ``min_distance`` peaks as seeds (h-maxima: ``utils/reconstruct.py``), anisotropic spacing (steps are
counted, not measured), gradients, multi-GPU forms, graph capture, int32 / float64 landscapes.
"""
import ctypes
import heapq

import numpy as np
import torch

from .. import _native as N
from . import _maps as M

__all__ = ["watershed"]

_COST, _SEED = 1, 2
DEFAULT_MAX_SWEEPS = 1 << 16         # per phase; a sweep moves a flood at least one tile on, so only a path that winds through more tiles gets here
_PHASES = ("cost", "path")


# ---------------------------------------------------------------------------------------------------------------- host form
def _offsets(dims, full):
    r = (-1, 0, 1)
    return [(dz, dy, dx) for dz in (r if dims == 3 else (0,)) for dy in r for dx in r
            if (dz, dy, dx) != (0, 0, 0) and (full or abs(dz) + abs(dy) + abs(dx) == 1)]


def _flood_entry(h, in_m, seed, dims, full):
    """``(C, sigma)`` of one entry ([D, H, W] arrays: float64 heights, the flooded set, the seeds) by ONE priority flood: the queue holds
    ``(pass height, steps, seed, position)``; a position is settled by the smallest entry that reaches it, and every settled position offers
    ``(max(C, h(n)), steps + 1, seed)`` to its open neighbours.  Lower pass heights are settled first, so all that steps into a level
    from below is queued before the level opens, and within a level the entries only grow with every step: the smallest entry of a
    position is the one the definition names."""
    D, H, W = h.shape
    PH, PW = H + 2, W + 2                                       # a closed border all round: no bounds checks below
    hp = np.full((D + 2, PH, PW), np.inf)
    hp[1:-1, 1:-1, 1:-1] = h
    closed = np.ones((D + 2, PH, PW), bool)
    closed[1:-1, 1:-1, 1:-1] = ~in_m
    hl, cl = hp.ravel().tolist(), bytearray(closed.ravel().tobytes())
    deltas = [(dz * PH + dy) * PW + dx for dz, dy, dx in _offsets(dims, full)]
    inner = np.arange((D + 2) * PH * PW).reshape(D + 2, PH, PW)[1:-1, 1:-1, 1:-1]
    cost = np.full(len(hl), np.inf)
    sigma = np.full(len(hl), -1, np.int64)
    heap = [(hl[p], 0, p, p) for p in inner[seed & in_m].tolist()]     # (the padded index orders the seeds as the linear index does)
    heapq.heapify(heap)
    pop, push = heapq.heappop, heapq.heappush
    while heap:
        c, d, s, p = pop(heap)
        if cl[p]:
            continue
        cl[p] = 1
        cost[p], sigma[p] = c, s
        for dl in deltas:
            n = p + dl
            if not cl[n]:
                hn = hl[n]
                push(heap, (c if c >= hn else hn, d + 1, s, n))
    cost, sigma = cost[inner], sigma[inner]
    z, r = np.divmod(np.maximum(sigma, 0), PH * PW)
    y, x = np.divmod(r, PW)
    return cost, np.where(sigma >= 0, ((z - 1) * H + (y - 1)) * W + (x - 1), -1)


def _host(height, markers, mask, B, D, H, W, dims, full, background, fill):
    h = height.contiguous().reshape(B, D, H, W).to(torch.float64).numpy()
    m = markers.contiguous().reshape(B, D, H, W).numpy()
    in_m = ~np.isnan(h) & (h != np.inf)
    if mask is not None:
        in_m &= mask.contiguous().reshape(B, D, H, W).numpy() != 0
    h = np.where(in_m, h, 0.0) + 0.0                            # (-0.0 + 0.0 is +0.0)
    seed = (m != background) if M.fits(background, markers.dtype) else np.ones(m.shape, bool)
    labels = np.empty_like(m)
    cost = np.empty(m.shape, np.float32)
    sigma = np.empty(m.shape, np.int32)
    for b in range(B):
        c, s = _flood_entry(h[b], in_m[b], seed[b], dims, full)
        cost[b], sigma[b] = c, s
        labels[b] = np.where(s >= 0, m[b].reshape(-1)[np.maximum(s, 0)], m.dtype.type(fill))
    shape = tuple(markers.shape)
    return torch.from_numpy(labels).reshape(shape), torch.from_numpy(cost).reshape(shape), torch.from_numpy(sigma).reshape(shape)


# ---------------------------------------------------------------------------------------------------------------- public
def _fill_value(background, dtype):
    """``background`` as a tensor of ``dtype`` holds it (itself where it fits; else truncated like a C cast, ``bool``: ``!= 0``)"""
    if M.fits(background, dtype):
        return background
    if dtype == torch.bool:
        return 1
    info = torch.iinfo(dtype)
    return (background - info.min) % (info.max - info.min + 1) + info.min


def watershed(height, markers, mask=None, connectivity=8, background=0, dims=2, return_cost=False, return_seed=False, return_sweeps=False,
              max_sweeps=None, out=None):
    """Flood ``height`` from the labelled positions of ``markers``: every position of the flooded set takes ``markers[sigma(p)]`` of the module
    docstring's definition -- the marker whose flood reaches it over the lowest pass, then in the fewest steps, then from the seed with the
    smallest linear index -- within its own stack entry.

    ``height``: a ``float32``, ``float16``, ``bfloat16``, ``uint8`` or ``int16`` tensor of shape ``[*stack, (D,) H, W]``; every value is exact in float32 and
    is widened as it is loaded (no float32 copy is made); ``-0.0`` counts as ``+0.0``.  ``markers``: an integer tensor (``bool``, ``uint8``, ``int16``, ``int32``,
    ``int64``) of the same shape on the same device; the result has its dtype.  ``mask``: ``bool`` / ``uint8`` of that shape, or ``None``.
    ``connectivity``: 4 or 8 for ``dims=2``, 6 or 26 for ``dims=3``.  At most 2^31 - 2 positions per call.

    THE FLOODED SET holds the positions where ``mask`` is non-zero and ``height`` is neither NaN nor ``+inf``.  Every position outside it, and every
    position no flood reaches, holds ``background`` in the result -- ALSO A LABELLED ONE: a seed outside the flooded set is not a seed and
    does not keep its value.  A ``background`` that markers' dtype cannot hold occurs nowhere: every position of the flooded set is a seed
    (and the positions outside it hold ``background`` truncated to the dtype).

    Further results, appended in this order: ``return_cost`` the float32 pass height ``C`` (``+inf`` where unreached); ``return_seed`` the int32
    ``sigma`` with ``nearest_site``'s index convention (``-1`` where unreached); ``return_sweeps`` a tuple of two ints, the sweeps the cost and the path
    phase took (``(0, 0)`` for CPU tensors and empty inputs).  ``out``: a tensor of markers' dtype, shape and device that receives the labels
    (and is returned); it may be ``markers`` itself.

    CUDA tensors: the kernels relax tile by tile until nothing changes, in sweeps launched eight at a time; after each batch one word is
    read back, so THE CALL SYNCHRONISES ITS STREAM AND CANNOT BE CAPTURED into a graph.  ``max_sweeps`` (default 65536) bounds the sweeps
    of each phase, the one that finds nothing left to do included; beyond it the call raises ``RuntimeError`` naming the phase and the
    count.  Contiguous inputs are read where they lie, whatever their alignment; other strides are copied first.  The result is a
    function of the inputs alone: the same bits on every run.  Bad arguments raise before anything is launched; empty inputs return
    without a launch."""
    what = "watershed"
    M.check_values(what, "height", height)
    M.check_labels(what, "markers", markers)
    connectivity, full = M.check_connectivity(what, connectivity, dims)
    _, B, D, H, W = M.extent(what, "labels", markers, dims, note=" (component numbers are int32)")      # (worded as connected_components words it)
    background = M.check_int(what, "background", background)
    dev = markers.device
    M.check_like(what, "height", height, markers)
    if mask is not None:
        M.check_like(what, "mask", mask, markers, (torch.bool, torch.uint8))
    max_sweeps = M.check_max_sweeps(what, max_sweeps, DEFAULT_MAX_SWEEPS)
    M.check_out(what, out, markers.dtype, markers)
    fill = _fill_value(background, markers.dtype)
    sweeps = (0, 0)
    if B * D * H * W == 0:
        res = out if out is not None else torch.empty(markers.shape, dtype=markers.dtype, device=dev)
        cost = torch.empty(markers.shape, dtype=torch.float32, device=dev)
        seed = torch.empty(markers.shape, dtype=torch.int32, device=dev)
    elif not markers.is_cuda:
        res, cost, seed = _host(height, markers, mask, B, D, H, W, dims, full, background, fill)
    else:
        x, h = markers.contiguous(), height.contiguous()
        m = mask.contiguous() if mask is not None else None
        flags = (_COST if return_cost else 0) | (_SEED if return_seed else 0)
        res = out if M.direct_out(out, x) else torch.empty(x.shape, dtype=x.dtype, device=dev)
        cost = torch.empty(x.shape, dtype=torch.float32, device=dev) if return_cost else None
        seed = torch.empty(x.shape, dtype=torch.int32, device=dev) if return_seed else None
        ws, nbytes = M.workspace(N.load().ptb_watershed_plan, what, dev, dims, B, D, H, W, flags)
        took = (ctypes.c_int * 2)(-1, -1)
        rc = N.launch("ptb_watershed", dev, h.data_ptr(), M.VALUE_CODES[h.dtype], x.data_ptr(), M.ELEM_BYTES[x.dtype], N.ptr(m), dims, B, D, H, W,
                      connectivity, background, fill, flags, max_sweeps, res.data_ptr(), N.ptr(cost), N.ptr(seed), took, ws.data_ptr(), nbytes,
                      raw=True)
        if rc == N.PTB_ENOTCONVERGED:
            M.raise_not_converged(what, _PHASES, took, max_sweeps)
        N.check(rc, what)
        sweeps = (int(took[0]), int(took[1]))
    res = M.finish_out(out, res)
    extra = ((cost,) if return_cost else ()) + ((seed,) if return_seed else ()) + ((sweeps,) if return_sweeps else ())
    return (res,) + extra if extra else res
