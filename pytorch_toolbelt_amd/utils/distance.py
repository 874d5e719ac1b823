"""Exact Euclidean distance transform of label maps, on the device the tensors are on: the step behind ``merge_crop(argmax=True)`` and
``connected_components`` that boundary / distance-map losses (the signed distance of the ground truth), the splitting of touching
instances (seeds are the maxima of the interior distance; ``utils/nearest.py`` grows them back) and every surface metric need.

The reference has no counterpart, so the names and meanings below are this library's; ``scipy.ndimage.distance_transform_edt`` is
the yardstick.  CUDA tensors run the HIP kernels of ``csrc/ptb_distance.hip`` (a missing kernel is an error, never a silent host
computation), CPU tensors take the numpy form below with the same results -- the device the caller names decides.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _native as N
from .components import _ELEM_BYTES, MAX_POSITIONS, _check_int, _fits

__all__ = ["distance_transform"]

MAX_SQUARED = (1 << 31) - 2          # D^2 + H^2 + W^2 of one call: every squared index distance is an int32
INT_INF = (1 << 31) - 1              # the int32 form of "no site in this entry"
_SITES_EQUAL, _SITES_NOT_EQUAL = 0, 1
_SQUARED, _SIGNED = 1, 2
_OUT_F32, _OUT_I32 = 0, 1
_HOST_INF = 1 << 62


# ---------------------------------------------------------------------------------------------------------------- validation
def _geometry(what, labels, dims):
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"{what}: labels must be a tensor, got {type(labels).__name__}")
    if labels.dtype not in _ELEM_BYTES:
        raise TypeError(f"{what}: labels must hold integer labels (bool, uint8, int16, int32 or int64), got {labels.dtype}")
    if dims not in (2, 3):
        raise ValueError(f"{what}: dims must be 2 or 3, got {dims!r}")
    if labels.dim() < dims:
        raise ValueError(f"{what}: labels must be [*stack, {'D, ' if dims == 3 else ''}H, W] for dims={dims}, got {tuple(labels.shape)}")
    D = labels.shape[-3] if dims == 3 else 1
    H, W = labels.shape[-2], labels.shape[-1]
    B = 1
    for s in labels.shape[:-dims]:
        B *= s
    if B * D * H * W > MAX_POSITIONS:
        raise ValueError(f"{what}: {B * D * H * W} positions in one call; at most 2^31 - 2 = {MAX_POSITIONS}: split the stack")
    squares = (D * D if dims == 3 else 0) + H * H + W * W
    if squares > MAX_SQUARED:
        raise ValueError(f"{what}: {'D^2 + ' if dims == 3 else ''}H^2 + W^2 = {squares}; at most 2^31 - 2 = {MAX_SQUARED} (squared index distances are int32)")
    return B, D, H, W


def _spacing(what, spacing, dims):
    if spacing is None:
        return None
    try:
        sp = [float(v) for v in spacing]
    except TypeError:
        raise TypeError(f"{what}: spacing must be None or {dims} floats in {'z, ' if dims == 3 else ''}y, x order, got {spacing!r}") from None
    if len(sp) != dims:
        raise ValueError(f"{what}: spacing must have {dims} entries ({'z, ' if dims == 3 else ''}y, x) for dims={dims}, got {len(sp)}")
    if not all(math.isfinite(v) and v > 0 for v in sp):
        raise ValueError(f"{what}: spacing must be positive and finite, got {sp}")
    return [1.0] * (3 - dims) + sp


# ---------------------------------------------------------------------------------------------------------------- host form
def _envelope_host(f, weight, inf):
    """``g[l, i] = min_j f[l, j] + weight * (i - j)^2`` of every line ``l`` of ``f`` ([lines, n]; ``inf`` marks "no value").  Correct rather than
    fast: the minimum is taken shift by shift, ``k = |i - j|`` = 1, 2, ... on both sides at once, over the lines that hold a value at all,
    and ends when ``weight * k^2`` is no smaller than the largest value that could still improve (an unreached position counts as ``inf``,
    so the shifts go on until every position of those lines is reached)."""
    live = (f != inf).any(axis=1)
    if not live.any():
        return f
    fl = f[live]
    gl = fl.copy()
    for k in range(1, f.shape[1]):
        c = weight * (k * k)
        if c >= gl.max():
            break
        np.minimum(gl[:, k:], fl[:, :-k] + c, out=gl[:, k:])
        np.minimum(gl[:, :-k], fl[:, k:] + c, out=gl[:, :-k])
    g = f.copy()
    g[live] = gl
    return g


def _squared_host(sites, sp):
    """squared distances to the sites of every entry of ``sites`` (bool [B, D, H, W]): int64 with ``_HOST_INF`` for unit spacing, float64 with
    ``inf`` otherwise"""
    if sp is None:
        inf = _HOST_INF
        f = np.where(sites, 0, inf).astype(np.int64)
        weights = (1, 1, 1)
    else:
        inf = np.inf
        f = np.where(sites, 0.0, inf)
        weights = tuple(s * s for s in sp)
    for axis in (3, 2, 1):
        if f.shape[axis] == 1:
            continue
        lines = np.ascontiguousarray(np.moveaxis(f, axis, -1))
        g = _envelope_host(lines.reshape(-1, lines.shape[-1]), weights[axis - 1], inf).reshape(lines.shape)
        f = np.moveaxis(g, -1, axis)
    return np.minimum(f, inf)


def _host(labels, B, D, H, W, sites_equal, value, sp, squared, signed):
    a = labels.reshape(B, D, H, W).numpy()
    if value is None:                                             # a value the dtype cannot hold occurs nowhere
        sites = np.zeros(a.shape, bool) if sites_equal else np.ones(a.shape, bool)
    else:
        sites = (a == value) if sites_equal else (a != value)

    def final(sq):
        if sp is None and squared:
            return np.minimum(sq, INT_INF)
        if sp is None:
            sq = np.where(sq >= _HOST_INF, np.inf, sq.astype(np.float64)).astype(np.float32)
        return sq if squared else np.sqrt(sq)

    res = final(_squared_host(sites, sp))
    if signed:
        res = final(_squared_host(~sites, sp)) - res
    return res.astype(np.int32 if sp is None and squared else np.float32)


# ---------------------------------------------------------------------------------------------------------------- public
def distance_transform(labels, background=0, foreground=None, dims=2, spacing=None, squared=False, signed=False, out=None):
    """The exact Euclidean distance of every position of ``labels`` to the nearest SITE of its own stack entry; 0 at sites.

    ``labels``: an integer tensor (``bool``, ``uint8``, ``int16``, ``int32``, ``int64``) of shape ``[*stack, H, W]`` (``dims=2``) or
    ``[*stack, D, H, W]`` (``dims=3``); the entries of ``stack`` are transformed independently, all in the same launches.  The sites are,
    with ``foreground=None``, the positions that hold ``background`` -- the result is scipy's ``distance_transform_edt(labels != background)``
    -- and with ``foreground=c`` the positions that do NOT hold ``c`` -- ``distance_transform_edt(labels == c)``, one class of a multi-class
    map without making ``labels == c``.  A ``background`` / ``foreground`` the dtype cannot hold occurs nowhere.

    ``spacing``: None for unit spacing, else ``dims`` positive finite floats in ``(z,) y, x`` order (scipy's ``sampling=``).  The result is
    float32; ``squared=True`` gives the squared distance instead, as exact **int32** with unit spacing and as float32 with ``spacing``.

    AN ENTRY WITHOUT ANY SITE gets ``inf`` (int32 form: 2^31 - 1).  This differs from scipy, which measures to a virtual site at index
    -1 there (a 3 x 4 map of ones gives 1, 1.41, 2.24, ...).

    ``signed=True``: ``d(position -> nearest position that is not a site) - d(position -> nearest site)``, the level-set convention of
    the boundary loss: positive on the sites (outside the object), negative inside; exactly one of the two terms is non-zero
    everywhere.  With ``squared=True``: that sign times d^2.  An entry that is all object gives ``-inf`` (int32: -(2^31 - 1)), one that is
    all sites ``+inf`` (2^31 - 1).  It costs two runs of the passes inside the one native call.

    ``out``: a tensor of the result's dtype, shape and device that receives the result (and is returned).

    The call is stream-ordered and reads nothing back.  Contiguous CUDA inputs are read where they lie (no boolean, widened or
    per-class copy); other strides are copied first.  The result is a function of the input alone: the same bits on every run.  More
    than 2^31 - 2 positions per call, or ``D^2 + H^2 + W^2 > 2^31 - 2``, raise ``ValueError`` before anything is launched; empty inputs
    return without a launch."""
    what = "distance_transform"
    B, D, H, W = _geometry(what, labels, dims)
    background = _check_int(what, "background", background, allow_none=True)
    foreground = _check_int(what, "foreground", foreground, allow_none=True)
    if foreground is None and background is None:
        raise ValueError(f"{what}: background=None needs foreground= (there would be no site to measure to)")
    sites_equal = foreground is None
    value = background if sites_equal else foreground
    sp = _spacing(what, spacing, dims)
    squared, signed = bool(squared), bool(signed)
    dtype = torch.int32 if squared and sp is None else torch.float32
    dev = labels.device
    if out is not None:
        if not isinstance(out, torch.Tensor):
            raise TypeError(f"{what}: out must be a tensor, got {type(out).__name__}")
        if out.dtype != dtype or out.shape != labels.shape or out.device != dev:
            raise ValueError(f"{what}: out must be a {dtype} tensor of shape {tuple(labels.shape)} on {dev}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    if B * D * H * W == 0:
        return out if out is not None else torch.empty(labels.shape, dtype=dtype, device=dev)
    if not labels.is_cuda:
        res = torch.from_numpy(_host(labels.contiguous(), B, D, H, W, sites_equal, value if _fits(value, labels.dtype) else None, sp, squared, signed))
        res = res.reshape(labels.shape)
    else:
        lib = N.load()
        x = labels.contiguous()
        nbytes = ctypes.c_int64()
        N.check(lib.ptb_edt_plan(dims, B, D, H, W, int(signed), ctypes.byref(nbytes)), what)
        with N.on_device(dev):
            res = out if out is not None and out.is_contiguous() and out.data_ptr() % 16 == 0 else torch.empty(x.shape, dtype=dtype, device=dev)
            ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
            N.bump()
            N.check(lib.ptb_edt(x.data_ptr(), _ELEM_BYTES[x.dtype], dims, B, D, H, W, _SITES_EQUAL if sites_equal else _SITES_NOT_EQUAL, value,
                                (ctypes.c_double * 3)(*sp) if sp is not None else None, (_SQUARED if squared else 0) | (_SIGNED if signed else 0),
                                res.data_ptr(), _OUT_I32 if dtype == torch.int32 else _OUT_F32, ws.data_ptr(), nbytes.value, N.stream_ptr(dev)), what)
    if out is None:
        return res
    if res is not out:
        out.copy_(res)
    return out
