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

__all__ = ["distance_transform", "class_distance_maps"]

MAX_SQUARED = (1 << 31) - 2          # D^2 + H^2 + W^2 of one call: every squared index distance is an int32
INT_INF = (1 << 31) - 1              # the int32 form of "no site in this entry"
_SITES_EQUAL, _SITES_NOT_EQUAL = 0, 1
_SQUARED, _SIGNED = 1, 2
_OUT_F32, _OUT_I32 = 0, 1
_HOST_INF = 1 << 62
PLANE_TRUTH, PLANE_PRED = 1, 2       # PTB_DLOSS_PLANE_*
DEFAULT_WORKSPACE_CAP = 4 << 30


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


# ---------------------------------------------------------------------------------------------------------------- per-class signed maps
_table_cache = {}


def class_table(what, classes, C, device=None):
    """``(K, classes tuple | None, host int array | None, device int32 [K + C] | None)`` of a class selection: the channel of every map, then
    for every channel its map or -1.  ``classes=None`` is all ``C`` channels in order and needs no table.  The device copy is made once
    per (classes, C, device), not per call."""
    if classes is None:
        return C, None, None, None
    try:
        cls = tuple(_check_int(what, "classes", int(c) if isinstance(c, torch.Tensor) else c) for c in classes)
    except TypeError:
        raise TypeError(f"{what}: classes must be None or a sequence of ints, got {classes!r}") from None
    if not cls:
        raise ValueError(f"{what}: classes must name at least one class")
    if len(set(cls)) != len(cls):
        raise ValueError(f"{what}: classes must be distinct, got {list(cls)}")
    if min(cls) < 0 or max(cls) >= C:
        raise ValueError(f"{what}: classes must lie in [0, {C}), got {list(cls)}")
    host = N.int_array(list(cls))
    if device is None or device.type != "cuda":
        return len(cls), cls, host, None
    key = (cls, C, str(device))
    dev = _table_cache.get(key)
    if dev is None:
        slot = [-1] * C
        for k, c in enumerate(cls):
            slot[c] = k
        if len(_table_cache) > 64:
            _table_cache.clear()
        dev = _table_cache[key] = torch.tensor(list(cls) + slot, dtype=torch.int32).to(device)
    return len(cls), cls, host, dev


def plan_maps(what, lib, dims, B, D, H, W, K, planes, cap):
    """``(entries per chunk, workspace bytes, partial slots)`` of ``ptb_dloss_plan``"""
    chunk, nbytes, least, slots = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    rc = lib.ptb_dloss_plan(dims, B, D, H, W, K, planes, cap, ctypes.byref(chunk), ctypes.byref(nbytes), ctypes.byref(least), ctypes.byref(slots))
    if rc == -1 and least.value > cap:
        raise ValueError(f"{what}: max_workspace_bytes={cap} is below the {least.value} bytes the transform of the smallest chunk of maps takes")
    if rc == N.PTB_EUNSUPPORTED:
        raise ValueError(f"{what}: a sample of {D * H * W} positions (or its squared extents) passes what one transform takes, 2^31 - 2")
    N.check(rc, what)
    return chunk.value, nbytes.value, slots.value


def signed_maps_device(what, x, labels, dense, C, table, planes, prob, has_ignore, ignore_label, ignore_value, dims, D, H, W, sp, squared, cap):
    """The signed maps ``[R, B, K, S]`` of the object maps one ``ptb_dloss_masks`` launch writes -- the truth plane, the thresholded
    prediction, or both (``planes``) -- by one ``ptb_edt`` call per chunk of entries.  ``x`` fp32 ``[B, C, S]`` (None for the truth plane
    alone); exactly one of ``labels`` int64 ``[B, S]`` / ``dense`` fp32 ``[B, C, S]``; ``C`` channels.  int32 with ``squared`` and unit spacing.  ``(maps, chunks)``."""
    lib = N.load()
    K, _, host, dev_table = table
    src = labels if labels is not None else dense
    B, S = src.shape[0], src.shape[-1]
    R = (planes & 1) + (planes >> 1)
    chunk, nbytes, _ = plan_maps(what, lib, dims, B, D, H, W, K, R, cap)
    E = R * B * K
    device = src.device
    as_int = squared and sp is None
    with N.on_device(device):
        masks = torch.empty(E * S, dtype=torch.uint8, device=device)
        maps = torch.empty((R, B, K, S), dtype=torch.int32 if as_int else torch.float32, device=device)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        stream = N.stream_ptr(device)
        N.bump()
        N.check(lib.ptb_dloss_masks(x.data_ptr() if x is not None else None, labels.data_ptr() if labels is not None else None,
                                    dense.data_ptr() if dense is not None else None, host, dev_table.data_ptr() if dev_table is not None else None,
                                    planes, B, C, K, S, prob, int(has_ignore), ignore_label, ignore_value, masks.data_ptr(), stream), what)
        spacing = (ctypes.c_double * 3)(*sp) if sp is not None else None
        flags = _SIGNED | (_SQUARED if squared else 0)
        chunks = 0
        for e0 in range(0, E, chunk):
            n = min(chunk, E - e0)
            N.bump()
            N.check(lib.ptb_edt(masks.data_ptr() + e0 * S, 1, dims, n, D, H, W, _SITES_EQUAL, 0, spacing, flags, maps.data_ptr() + 4 * e0 * S,
                                _OUT_I32 if as_int else _OUT_F32, ws.data_ptr(), nbytes, stream), what)
            chunks += 1
    return maps, chunks


def signed_maps_host(objects, sp, squared):
    """The same maps of the boolean numpy array ``objects`` ``[E, D, H, W]``: what ``distance_transform(signed=True)`` gives with the
    positions outside an object as its sites"""
    E, D, H, W = objects.shape
    return _host(torch.from_numpy(np.ascontiguousarray(objects).astype(np.uint8)), E, D, H, W, True, 0, sp, squared, True)


def class_distance_maps(labels, num_classes=None, classes=None, dims=2, spacing=None, ignore_index=None, squared=False,
                        max_workspace_bytes=DEFAULT_WORKSPACE_CAP):
    """The SIGNED distance map of every class of a batch of label maps: what the distance-map losses (``losses.BoundaryLoss``,
    ``losses.HausdorffDTLoss``) take as ``dist_maps=`` -- computed once per dataset, on the device, instead of once per step.

    ``labels``: an integer tensor ``[B, H, W]`` (``dims=2``) or ``[B, D, H, W]`` (``dims=3``).  The K maps of a sample are those of
    ``classes`` (distinct ints in ``[0, num_classes)``, in that order), or of all ``num_classes`` classes; ``num_classes=None`` takes
    ``max(classes) + 1``.  Returns ``[B, K, *spatial]``: map ``k`` is ``distance_transform(labels, foreground=classes[k], signed=True,
    spacing=..., squared=...)``, bit for bit -- positive outside the object, negative inside (the boundary positions inside hold -1, not
    0), float32, or exact int32 with ``squared=True`` and unit spacing.  Positions that hold ``ignore_index`` belong to no class.

    THE INFINITIES STAY: a sample without class ``k`` has ``+inf`` (int32: 2^31 - 1) in all of map ``k``, a sample that is class ``k``
    everywhere ``-inf``.  The losses count such a map as 0 (it has no boundary); anything else that reads the maps must decide itself.

    One launch writes all ``B * K`` object maps (uint8), then one distance transform runs per chunk of them; the chunks keep the
    transform's workspace (12 bytes per position, 16 for ``dims=3``) within ``max_workspace_bytes`` and change no bit.  Stream-ordered,
    nothing is read back.  CPU tensors take the numpy form with the same results.  For the losses pass ``squared=True`` with unit
    spacing (the exact integers they use internally) and the distances themselves with ``spacing``."""
    what = "class_distance_maps"
    if not isinstance(labels, torch.Tensor) or labels.dtype not in _ELEM_BYTES:
        raise TypeError(f"{what}: labels must be an integer tensor (bool, uint8, int16, int32 or int64)")
    if dims not in (2, 3):
        raise ValueError(f"{what}: dims must be 2 or 3, got {dims!r}")
    if labels.dim() != dims + 1:
        raise ValueError(f"{what}: labels must be [B, {'D, ' if dims == 3 else ''}H, W] for dims={dims}, got {tuple(labels.shape)}")
    num_classes = _check_int(what, "num_classes", num_classes, allow_none=True)
    if num_classes is None:
        if classes is None:
            raise ValueError(f"{what}: give num_classes= or classes=")
        num_classes = max(int(c) for c in classes) + 1 if len(classes) else 1
    if not 1 <= num_classes < (1 << 31):
        raise ValueError(f"{what}: num_classes must be positive, got {num_classes}")
    ignore_index = _check_int(what, "ignore_index", ignore_index, allow_none=True)
    cap = _check_int(what, "max_workspace_bytes", max_workspace_bytes)
    if cap < 0:
        raise ValueError(f"{what}: max_workspace_bytes must not be negative, got {cap}")
    sp = _spacing(what, spacing, dims)
    squared = bool(squared)
    table = class_table(what, classes, num_classes, labels.device)
    K, cls = table[0], table[1] if table[1] is not None else tuple(range(num_classes))
    B = labels.shape[0]
    spatial = tuple(labels.shape[1:])
    D = spatial[0] if dims == 3 else 1
    H, W = spatial[-2], spatial[-1]
    _geometry(what, labels[:1] if B else labels, dims)
    dtype = torch.int32 if squared and sp is None else torch.float32
    if B * D * H * W == 0:
        return torch.empty((B, K) + spatial, dtype=dtype, device=labels.device)
    lab = labels.reshape(B, -1).to(torch.int64).contiguous()
    if not labels.is_cuda:
        a = lab.numpy().reshape(B, 1, D, H, W)
        objects = a == np.asarray(cls, dtype=np.int64).reshape(1, K, 1, 1, 1)
        if ignore_index is not None:
            objects &= a != ignore_index
        return torch.from_numpy(signed_maps_host(objects.reshape(B * K, D, H, W), sp, squared)).reshape((B, K) + spatial)
    maps, _ = signed_maps_device(what, None, lab, None, num_classes, table, PLANE_TRUTH, 2, ignore_index is not None, ignore_index or 0, 0.0, dims, D, H, W, sp,
                                 squared, cap)
    return maps.reshape((B, K) + spatial)
