"""Morphological reconstruction and what is built on it, on the device the tensors are on: grey reconstruction by dilation and erosion,
regional maxima / minima, h-maxima / h-minima and hole filling -- the seed finder and the clean-up step of the instance chain::

    sem = fill_holes(sem)                                                  # close the holes of a predicted mask
    d = distance_transform(sem)
    cores, n = connected_components(h_maxima(d, 2.0, domain=sem != 0))     # one core per object: no global radius to tune
    inst = watershed(-d, cores, mask=sem != 0)

The threshold recipe ``distance_transform(sem) > r`` needs one ``r`` for all objects: a small one leaves touching large objects in one core,
a large one deletes small objects.  ``h_maxima`` keeps every peak of the distance map that stands more than ``h`` above the pass to a
higher one, whatever its size.  The reference has no counterpart, so the names and meanings below are this library's.  CUDA tensors run
the HIP kernels of ``csrc/ptb_reconstruct.hip`` (a missing kernel is an error, never a silent host computation), CPU tensors take the host
form below with the same bits -- the device the caller names decides.

DEFINITIONS.  Tensors are ``[*stack, H, W]`` (``dims=2``) or ``[*stack, D, H, W]`` (``dims=3``); stack entries are independent.

THE DOMAIN holds the positions where ``domain`` is non-zero (all positions, if ``domain`` is ``None``) and the mask / image is not NaN.  Positions
outside the domain are never neighbours; there ``reconstruction`` and ``fill_holes`` return the mask's / image's own value and the extrema
return False.  A NaN in ``seed`` counts as the lowest value (erosion: the highest, and comes back as ``-inf`` / ``+inf`` where nothing raises
it).  ``+-inf`` are ordinary values.  ``-0`` counts as ``+0`` and comes back as ``+0``.

``reconstruction(seed, mask)``, dilation: with ``s = min(seed, mask)``, ``R(p)`` is the maximum over the paths of the domain that end at ``p`` of
``min(s(start), min of mask along the path)`` -- the least fixed point of ``R(p) <- max(R(p), min(R(q), mask(p)))`` over neighbours ``q``, taken
from ``s``.  ``min`` and ``max`` only select input values, so the result has the inputs' dtype exactly and no order or tie rule enters it.
Erosion is the mirror image (computed on complemented keys, not by a second kernel).  DIVERGENCE FROM skimage: where ``seed > mask`` the
seed is clamped to the mask (skimage raises), because a check would need a read-back.

``regional_maxima(image)``: True on the plateaus -- connected sets of equal values -- without a strictly higher neighbour.  Computed as
``R(image-, image) < image`` with ``image-`` the image lowered by ONE STEP OF THE ORDERED 32-BIT KEY of its float32 value (the smallest key of a
value is 0x007FFFFF, so the step cannot underflow).  A constant entry is ONE maximum (skimage returns none there).

``h_maxima(image, h)``: ``HMAX = R(float32(image) - float32(h), image)`` -- one float32 subtraction, clamped -- and then ``regional_maxima(HMAX)``:
the maxima whose dynamic is STRICTLY greater than ``h`` (Soille's definition), each grown to the plateau of ``HMAX`` that the cut leaves of it.
Two relaxation phases in one native call.  skimage's ``h_maxima`` thresholds a residue instead and can differ where the dynamic equals ``h``.
``h_minima`` and ``regional_minima`` are the mirror images.  Example, 4 neighbours, one row ``[0, 1, 3, 5, 3, 2, 2.5, 3, 2.5, 1, 0]``: ``h = 0.5`` gives
``[0,0,0,1,0,0,1,1,1,0,0]``, ``h = 1`` and ``h = 1.5`` give ``[0,0,0,1,0,0,0,0,0,0,0]``, ``h = 3.5`` gives ``[0,0,1,1,1,1,1,1,1,0,0]``.

``fill_holes(image)``: reconstruction by erosion from a start that holds the image's own value on the faces of the entry (the array
border) and the highest value elsewhere.  On a 0/1 mask it equals ``scipy.ndimage.binary_fill_holes`` with the matching structure.  Only
the array border is open: a position next to the outside of ``domain`` is not.  A domain position that no face reaches holds the highest
value of the dtype (``+inf``, 255, 32767, True).

Left out: structuring-element erosion / dilation filters, ``clear_border``, ``min_distance`` peaks, anisotropy, gradients, multi-GPU forms,
graph capture, int32 / float64 images.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _native as N
from . import _maps as M

__all__ = ["reconstruction", "regional_maxima", "regional_minima", "h_maxima", "h_minima", "fill_holes"]

_VALUES, _EXTREMA, _H_EXTREMA, _FILL = range(4)             # PTB_RECONSTRUCT_*
_CODES = {**M.VALUE_CODES, torch.bool: N.U8}
_TOP = {torch.float32: math.inf, torch.float16: math.inf, torch.bfloat16: math.inf, torch.uint8: 255.0, torch.int16: 32767.0, torch.bool: 1.0}
DEFAULT_MAX_SWEEPS = 1 << 16         # per phase; a sweep carries a value at least one tile on, so only a path that winds through more tiles gets here
_PHASES = {_VALUES: ("reconstruction",), _EXTREMA: ("regional-extrema",), _H_EXTREMA: ("h-reconstruction", "regional-extrema"), _FILL: ("hole-filling",)}
_LOWEST = 0x007FFFFF                 # the smallest key of a value; 0 is the key of a position outside the domain


# ---------------------------------------------------------------------------------------------------------------- host form
def _keys(v, flip):
    """the ordered 32-bit keys of a float32 array (int64, so that a step down needs no care): monotone, -0 as +0; ``flip``: complemented"""
    b = np.where(v == 0, np.uint32(0), v.view(np.uint32))
    k = np.where(b & np.uint32(0x80000000) != 0, ~b, b | np.uint32(0x80000000))
    return (k ^ np.uint32(flip)).astype(np.int64)


def _unkeys(k, flip):
    k = k.astype(np.uint32) ^ np.uint32(flip)
    return np.where(k & np.uint32(0x80000000) != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _spread(a):
    """the maximum over the 3-window along every axis behind the first (the stack): what a slice offers the next slice, full neighbourhood"""
    for ax in range(1, a.ndim):
        if a.shape[ax] > 1:
            lo = [slice(None)] * a.ndim
            hi = [slice(None)] * a.ndim
            lo[ax], hi[ax] = slice(None, -1), slice(1, None)
            b = a.copy()
            np.maximum(b[tuple(hi)], a[tuple(lo)], out=b[tuple(hi)])
            np.maximum(b[tuple(lo)], a[tuple(hi)], out=b[tuple(lo)])
            a = b
    return a


def _relax(r, m, dims, full):
    """the least fixed point of ``r <- max(r, min(r(q), m))`` above ``r``, in place: ``[B, *spatial]`` key arrays.  Directional sweeps -- along every axis,
    up and down, a slice taking what the slice before it offers -- until a round changes nothing.  Every step keeps ``r`` below the fixed
    point and a round without a change is one, so the order of the sweeps does not enter the result."""
    while True:
        before = r.copy()
        for ax in range(1, dims + 1):
            rm, mm = np.moveaxis(r, ax, 0), np.moveaxis(m, ax, 0)
            n = rm.shape[0]
            for i, j in [(i, i - 1) for i in range(1, n)] + [(i, i + 1) for i in range(n - 2, -1, -1)]:
                offer = _spread(rm[j]) if full else rm[j]
                np.maximum(rm[i], np.minimum(offer, mm[i]), out=rm[i])
        if np.array_equal(before, r):
            return r


def _faces(shape, dims):
    f = np.zeros(shape, bool)
    for ax in range(1, dims + 1):
        for at in (0, -1):
            f[(slice(None),) * ax + (at,)] = True
    return f


def _host(op, erosion, seed, mask, domain, h, dims, full, shape3, out_dtype):
    flip = 0xFFFFFFFF if erosion else 0
    v = mask.contiguous().reshape(shape3).to(torch.float32).numpy()
    inside = ~np.isnan(v)
    if domain is not None:
        inside &= domain.contiguous().reshape(shape3).numpy() != 0
    m = np.where(inside, _keys(v, flip), 0)
    if op == _VALUES:
        s = seed.contiguous().reshape(shape3).to(torch.float32).numpy()
        start = np.where(np.isnan(s), _LOWEST, _keys(s, flip))
    elif op == _EXTREMA:
        start = m - 1
    elif op == _H_EXTREMA:
        with np.errstate(invalid="ignore", over="ignore"):
            start = _keys(v + np.float32(h) if erosion else v - np.float32(h), flip)
    else:
        start = np.where(_faces(shape3, dims), m, _LOWEST)
    r = _relax(np.where(inside, np.minimum(start, m), 0), m, dims, full)
    if op == _H_EXTREMA:
        m = r
        r = _relax(np.where(inside, m - 1, 0), m, dims, full)
    if op in (_EXTREMA, _H_EXTREMA):
        return torch.from_numpy(r < m)
    with np.errstate(invalid="ignore"):                         # (key 0 maps back to a NaN: replaced below)
        vals = torch.from_numpy(np.minimum(_unkeys(r, flip), np.float32(_TOP[out_dtype])))
    return torch.where(torch.from_numpy(inside), vals.to(out_dtype), mask.contiguous().reshape(shape3))


# ---------------------------------------------------------------------------------------------------------------- public
def _run(what, op, erosion, seed, mask, name, h, connectivity, domain, dims, out, max_sweeps, return_sweeps, default_full=True):
    M.check_values(what, name, mask, or_bool=op == _FILL)
    connectivity, full = M.check_connectivity(what, connectivity, dims, default=1 if default_full else 0, note=" (or None)")
    _, B, D, H, W = M.extent(what, name, mask, dims)
    dev = mask.device
    if seed is not None:
        M.check_values(what, "seed", seed)
        if seed.dtype != mask.dtype:
            raise TypeError(f"{what}: seed and mask must have the same dtype, got {seed.dtype} and {mask.dtype}")
        M.check_like(what, "seed", seed, mask)
    if domain is not None:
        M.check_like(what, "domain", domain, mask, (torch.bool, torch.uint8))
    if op == _H_EXTREMA:
        if isinstance(h, (bool, np.bool_)) or not isinstance(h, (int, float, np.integer, np.floating)):
            raise TypeError(f"{what}: h must be a number, got {h!r}")
        with np.errstate(over="ignore"):
            h = float(np.float32(h))
        if not (h >= 0.0 and math.isfinite(h)):
            raise ValueError(f"{what}: h must be finite and >= 0 in float32, got {h!r}")
    max_sweeps = M.check_max_sweeps(what, max_sweeps, DEFAULT_MAX_SWEEPS)
    out_dtype = torch.bool if op in (_EXTREMA, _H_EXTREMA) else mask.dtype
    M.check_out(what, out, out_dtype, mask)
    sweeps = (0, 0)
    if B * D * H * W == 0:
        res = out if out is not None else torch.empty(mask.shape, dtype=out_dtype, device=dev)
    elif not mask.is_cuda:
        res = _host(op, erosion, seed, mask, domain, h, dims, full, (B,) + tuple(mask.shape[mask.dim() - dims:]), out_dtype).reshape(mask.shape)
    else:
        m = mask.contiguous()
        s = seed.contiguous() if seed is not None else None
        k = domain.contiguous() if domain is not None else None
        res = out if M.direct_out(out, m, s, k) else torch.empty(m.shape, dtype=out_dtype, device=dev)
        ws, nbytes = M.workspace(N.load().ptb_reconstruct_plan, what, dev, dims, B, D, H, W, op)
        took = (ctypes.c_int * 2)(-1, -1)
        rc = N.launch("ptb_reconstruct", dev, N.ptr(s), m.data_ptr(), _CODES[m.dtype], N.ptr(k), dims, B, D, H, W, connectivity, op, int(erosion),
                      h if op == _H_EXTREMA else 0.0, _TOP[m.dtype] if op == _FILL else math.inf, max_sweeps,
                      res.data_ptr(), took, ws.data_ptr(), nbytes, raw=True)    # (a bool tensor's bytes are the uint8 the kernels read)
        if rc == N.PTB_ENOTCONVERGED:
            M.raise_not_converged(what, _PHASES[op], took, max_sweeps)
        N.check(rc, what)
        sweeps = (int(took[0]), max(int(took[1]), 0))
    res = M.finish_out(out, res)
    return (res, sweeps) if return_sweeps else res


_COMMON = """``connectivity``: 4 or 8 for ``dims=2``, 6 or 26 for ``dims=3``; ``None``: {default}.  ``domain``: ``bool`` / ``uint8`` of the same shape on the same
    device, or ``None`` (see the module docstring for what lies outside it).  Value dtypes: ``float32``, ``float16``, ``bfloat16``, ``uint8``, ``int16``{also}, read
    where they lie and widened on load; other strides are copied first.  At most 2^31 - 2 positions per call.  ``out``: a tensor of the
    result's dtype, shape and device that receives the result (and is returned); it may be an input.  ``return_sweeps``: also return a tuple
    of two ints, the sweeps each relaxation phase took (0 for a phase the operation does not have, for CPU tensors and for empty inputs).

    CUDA tensors: ONE native call; the kernels relax tile by tile until nothing changes, in sweeps launched eight at a time on the caller's
    stream; after each batch one word is read back, so THE CALL SYNCHRONISES ITS STREAM AND CANNOT BE CAPTURED into a graph.  ``max_sweeps``
    (default 65536) bounds the sweeps of each phase, the one that finds nothing left to do included; beyond it the call raises
    ``RuntimeError`` naming the phase and the count.  The result is a function of the inputs alone: the same bits on every run.  Bad
    arguments raise before anything is launched; empty inputs return without a launch."""


def reconstruction(seed, mask, method="dilation", connectivity=None, domain=None, dims=2, out=None, max_sweeps=None, return_sweeps=False):
    """Grey reconstruction of ``mask`` from ``seed`` by ``method`` ``"dilation"`` or ``"erosion"`` (the module docstring's definition): ``seed`` and ``mask`` of one
    dtype, shape and device; the result has that dtype.  Where ``seed > mask`` (erosion: ``<``) the seed is clamped.

    """
    if method not in ("dilation", "erosion"):
        raise ValueError(f"reconstruction: method must be 'dilation' or 'erosion', got {method!r}")
    if not isinstance(seed, torch.Tensor):
        raise TypeError(f"reconstruction: seed must be a tensor, got {type(seed).__name__}")
    return _run("reconstruction", _VALUES, method == "erosion", seed, mask, "mask", 0.0, connectivity, domain, dims, out, max_sweeps, return_sweeps)


def regional_maxima(image, connectivity=None, domain=None, dims=2, out=None, max_sweeps=None, return_sweeps=False):
    """The bool map of the regional maxima of ``image``: the plateaus without a strictly higher neighbour.  A constant entry is one maximum.

    """
    return _run("regional_maxima", _EXTREMA, False, None, image, "image", 0.0, connectivity, domain, dims, out, max_sweeps, return_sweeps)


def regional_minima(image, connectivity=None, domain=None, dims=2, out=None, max_sweeps=None, return_sweeps=False):
    """The bool map of the regional minima of ``image``: the mirror image of ``regional_maxima``.

    """
    return _run("regional_minima", _EXTREMA, True, None, image, "image", 0.0, connectivity, domain, dims, out, max_sweeps, return_sweeps)


def h_maxima(image, h, connectivity=None, domain=None, dims=2, out=None, max_sweeps=None, return_sweeps=False):
    """The bool map of the extended maxima of ``image`` at height ``h >= 0``: the regional maxima of the reconstruction of ``image`` from
    ``float32(image) - float32(h)`` -- the maxima whose dynamic is strictly greater than ``h``.  ``h = 0`` gives ``regional_maxima(image)``.

    """
    return _run("h_maxima", _H_EXTREMA, False, None, image, "image", h, connectivity, domain, dims, out, max_sweeps, return_sweeps)


def h_minima(image, h, connectivity=None, domain=None, dims=2, out=None, max_sweeps=None, return_sweeps=False):
    """The bool map of the extended minima of ``image`` at depth ``h >= 0``: the mirror image of ``h_maxima`` (``float32(image) + float32(h)``).

    """
    return _run("h_minima", _H_EXTREMA, True, None, image, "image", h, connectivity, domain, dims, out, max_sweeps, return_sweeps)


def fill_holes(image, connectivity=None, domain=None, dims=2, out=None, max_sweeps=None, return_sweeps=False):
    """Fill the holes of a ``bool`` / ``uint8`` mask or of a grey image: every position takes the lowest level at which a flood from the array
    border reaches it.  ``connectivity`` is that of the FLOOD (of the background); the default is the minimal one, like the default
    structure of ``scipy.ndimage.binary_fill_holes``, which the result equals on 0/1 masks.  The result has the image's dtype.

    """
    return _run("fill_holes", _FILL, True, None, image, "image", 0.0, connectivity, domain, dims, out, max_sweeps, return_sweeps, default_full=False)


for _f, _d, _a in ((reconstruction, "the full neighbourhood (8 / 26)", ""), (regional_maxima, "the full neighbourhood (8 / 26)", ""),
                   (regional_minima, "the full neighbourhood (8 / 26)", ""), (h_maxima, "the full neighbourhood (8 / 26)", ""),
                   (h_minima, "the full neighbourhood (8 / 26)", ""), (fill_holes, "the minimal one (4 / 6)", " and ``bool``")):
    _f.__doc__ += _COMMON.format(default=_d, also=_a)
