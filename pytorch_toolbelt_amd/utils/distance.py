"""Exact Euclidean distance transform of label maps, on the device the tensors are on: the step behind ``merge_crop(argmax=True)`` and
``connected_components`` that boundary / distance-map losses (the signed distance of the ground truth), the splitting of touching
instances (seeds are the maxima of the interior distance; ``utils/nearest.py`` grows them back) and every surface metric need.

The reference has no counterpart, so the names and meanings below are this library's; ``scipy.ndimage.distance_transform_edt`` is
the yardstick.  CUDA tensors run the HIP kernels of ``csrc/ptb_distance.hip`` (a missing kernel is an error, never a silent host
computation), CPU tensors take the numpy form below with the same results -- the device the caller names decides.
"""
import ctypes

import numpy as np
import torch

from .. import _native as N
from . import _maps as M

__all__ = ["distance_transform", "class_distance_maps"]

MAX_POSITIONS, MAX_SQUARED, INT_INF = M.MAX_POSITIONS, M.MAX_SQUARED, M.INT_INF
_SQUARED, _SIGNED = 1, 2
_OUT_F32, _OUT_I32 = 0, 1
PLANE_TRUTH, PLANE_PRED = 1, 2       # PTB_DLOSS_PLANE_*
DEFAULT_WORKSPACE_CAP = 4 << 30


# ---------------------------------------------------------------------------------------------------------------- host form
def _squared_host(sites, sp):
    """squared distances to the sites of every entry of ``sites`` (bool [B, D, H, W]): int64 with ``HOST_INF`` for unit spacing, float64 with
    ``inf`` otherwise"""
    return M.edt_host(sites, sp)[0]


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
            sq = np.where(sq >= M.HOST_INF, np.inf, sq.astype(np.float64)).astype(np.float32)
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
    M.check_labels(what, "labels", labels)
    _, B, D, H, W = M.extent(what, "labels", labels, dims, squares=True)
    background = M.check_int(what, "background", background, allow_none=True)
    foreground = M.check_int(what, "foreground", foreground, allow_none=True)
    if foreground is None and background is None:
        raise ValueError(f"{what}: background=None needs foreground= (there would be no site to measure to)")
    sites_equal = foreground is None
    value = background if sites_equal else foreground
    sp = M.spacing(what, spacing, dims)
    squared, signed = bool(squared), bool(signed)
    dtype = torch.int32 if squared and sp is None else torch.float32
    dev = labels.device
    M.check_out(what, out, dtype, labels)
    if B * D * H * W == 0:
        return out if out is not None else torch.empty(labels.shape, dtype=dtype, device=dev)
    if not labels.is_cuda:
        res = torch.from_numpy(_host(labels.contiguous(), B, D, H, W, sites_equal, value if M.fits(value, labels.dtype) else None, sp, squared, signed))
        res = res.reshape(labels.shape)
    else:
        x = labels.contiguous()
        res = out if M.direct_out(out) else torch.empty(x.shape, dtype=dtype, device=dev)
        ws, nbytes = M.workspace(N.load().ptb_edt_plan, what, dev, dims, B, D, H, W, int(signed))
        N.launch("ptb_edt", dev, x.data_ptr(), M.ELEM_BYTES[x.dtype], dims, B, D, H, W, M.SITES_EQUAL if sites_equal else M.SITES_NOT_EQUAL, value,
                 (ctypes.c_double * 3)(*sp) if sp is not None else None, (_SQUARED if squared else 0) | (_SIGNED if signed else 0),
                 res.data_ptr(), _OUT_I32 if dtype == torch.int32 else _OUT_F32, ws.data_ptr(), nbytes, what=what)
    return M.finish_out(out, res)


# ---------------------------------------------------------------------------------------------------------------- per-class signed maps
_table_cache = {}


def class_table(what, classes, C, device=None):
    """``(K, classes tuple | None, host int array | None, device int32 [K + C] | None)`` of a class selection: the channel of every map, then
    for every channel its map or -1.  ``classes=None`` is all ``C`` channels in order and needs no table.  The device copy is made once
    per (classes, C, device), not per call."""
    if classes is None:
        return C, None, None, None
    try:
        cls = tuple(M.check_int(what, "classes", int(c) if isinstance(c, torch.Tensor) else c) for c in classes)
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
    K, _, host, dev_table = table
    src = labels if labels is not None else dense
    B, S = src.shape[0], src.shape[-1]
    R = (planes & 1) + (planes >> 1)
    chunk, nbytes, _ = plan_maps(what, N.load(), dims, B, D, H, W, K, R, cap)
    E = R * B * K
    device = src.device
    as_int = squared and sp is None
    masks = torch.empty(E * S, dtype=torch.uint8, device=device)
    maps = torch.empty((R, B, K, S), dtype=torch.int32 if as_int else torch.float32, device=device)
    ws = M.scratch(nbytes, device)
    N.launch("ptb_dloss_masks", device, N.ptr(x), N.ptr(labels), N.ptr(dense), host, N.ptr(dev_table), planes, B, C, K, S, prob, int(has_ignore),
             ignore_label, ignore_value, masks.data_ptr(), what=what)
    spacing = (ctypes.c_double * 3)(*sp) if sp is not None else None
    flags = _SIGNED | (_SQUARED if squared else 0)
    chunks = 0
    for e0 in range(0, E, chunk):
        n = min(chunk, E - e0)
        N.launch("ptb_edt", device, masks.data_ptr() + e0 * S, 1, dims, n, D, H, W, M.SITES_EQUAL, 0, spacing, flags, maps.data_ptr() + 4 * e0 * S,
                 _OUT_I32 if as_int else _OUT_F32, ws.data_ptr(), nbytes, what=what)
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
    if not isinstance(labels, torch.Tensor) or labels.dtype not in M.ELEM_BYTES:
        raise TypeError(f"{what}: labels must be an integer tensor (bool, uint8, int16, int32 or int64)")
    M.check_dims(what, dims)
    if labels.dim() != dims + 1:
        raise ValueError(f"{what}: labels must be [B, {'D, ' if dims == 3 else ''}H, W] for dims={dims}, got {tuple(labels.shape)}")
    num_classes = M.check_int(what, "num_classes", num_classes, allow_none=True)
    if num_classes is None:
        if classes is None:
            raise ValueError(f"{what}: give num_classes= or classes=")
        num_classes = max(int(c) for c in classes) + 1 if len(classes) else 1
    if not 1 <= num_classes < (1 << 31):
        raise ValueError(f"{what}: num_classes must be positive, got {num_classes}")
    ignore_index = M.check_int(what, "ignore_index", ignore_index, allow_none=True)
    cap = M.check_int(what, "max_workspace_bytes", max_workspace_bytes)
    if cap < 0:
        raise ValueError(f"{what}: max_workspace_bytes must not be negative, got {cap}")
    sp = M.spacing(what, spacing, dims)
    squared = bool(squared)
    table = class_table(what, classes, num_classes, labels.device)
    K, cls = table[0], table[1] if table[1] is not None else tuple(range(num_classes))
    B = labels.shape[0]
    spatial = tuple(labels.shape[1:])
    D = spatial[0] if dims == 3 else 1
    H, W = spatial[-2], spatial[-1]
    M.extent(what, "labels", labels[:1] if B else labels, dims, squares=True)
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
