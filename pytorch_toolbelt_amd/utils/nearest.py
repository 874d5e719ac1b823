"""Nearest-site feature transform and label expansion, on the device the tensors are on: which site ``distance_transform`` measures to,
not only how far it is -- scipy's ``distance_transform_edt(return_indices=True)`` -- and on top of it the step that splits touching
instances: ``skimage.segmentation.expand_labels`` with a mask::

    cores, n = connected_components(distance_transform(sem) > r)     # one core per object
    inst = expand_labels(cores, mask=sem != 0)                       # every object pixel takes the label of its nearest core

The reference has no counterpart, so the names and meanings below are this library's.  CUDA tensors run the HIP kernels of
``csrc/ptb_nearest.hip`` (a missing kernel is an error, never a silent host computation), CPU tensors take the numpy form below with
the same results -- the device the caller names decides.

THE TIE RULE.  Among all sites at the minimum squared distance the one with the SMALLEST LINEAR INDEX is returned.  The rule does not
depend on the order of anything: every pass prefers the smaller coordinate of its axis on a tie, and the axes are passed from the
fastest to the slowest.  scipy breaks ties otherwise, so its indices are a yardstick for the distance they imply, not for the index.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _native as N
from . import _maps as M

__all__ = ["nearest_site", "expand_labels"]

_INDEX, _SQUARED, _GATHER, _MAX_SQ = 1, 2, 4, 8


# ---------------------------------------------------------------------------------------------------------------- host form
def _feature_host(sites, sp):
    """``(squared distance, index of the nearest site within the entry)`` of every position of ``sites`` (bool [B, D, H, W]): int64 with
    ``HOST_INF`` for unit spacing, float64 with ``inf`` otherwise; int64 indices, -1 without a site"""
    return M.edt_host(sites, sp, index=True)


def _sites_host(labels, B, D, H, W, sites_equal, value):
    a = labels.reshape(B, D, H, W).numpy()
    if value is None:                                             # a value the dtype cannot hold occurs nowhere
        return np.zeros(a.shape, bool) if sites_equal else np.ones(a.shape, bool)
    return (a == value) if sites_equal else (a != value)


def _squared_form(sq, sp):
    """the stored form of the squared distances: int32 with INT_INF for unit spacing, float32 otherwise"""
    return np.minimum(sq, M.INT_INF).astype(np.int32) if sp is None else sq.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- native call
def _native(what, x, dims, B, D, H, W, sites_equal, value, sp, flags, index=None, squared=None, gather=None, mask=None, max_sq=0.0):
    ws, nbytes = M.workspace(N.load().ptb_nearest_plan, what, x.device, dims, B, D, H, W, flags)
    N.launch("ptb_nearest", x.device, x.data_ptr(), M.ELEM_BYTES[x.dtype], dims, B, D, H, W, M.SITES_EQUAL if sites_equal else M.SITES_NOT_EQUAL, value,
             (ctypes.c_double * 3)(*sp) if sp is not None else None, flags, N.ptr(index), N.ptr(squared), N.ptr(gather), N.ptr(mask), max_sq,
             ws.data_ptr(), nbytes, what=what)


# ---------------------------------------------------------------------------------------------------------------- public
def nearest_site(labels, background=0, foreground=None, dims=2, spacing=None, return_distance=False, out=None):
    """The nearest SITE of every position of ``labels`` within its own stack entry, as an **int32** tensor of ``labels.shape`` that holds
    the site's linear index ``(z * H + y) * W + x`` counted within the entry (``numpy.unravel_index`` gives scipy's ``return_indices``
    form).  A site gets its own index; every position of AN ENTRY WITHOUT ANY SITE gets ``-1``.

    ``labels``, ``background`` / ``foreground``, ``dims`` and ``spacing`` mean what they mean in ``distance_transform``: the sites are, with
    ``foreground=None``, the positions that hold ``background`` and with ``foreground=c`` the positions that do not hold ``c``; the limits
    are the same (2^31 - 2 positions per call, ``D^2 + H^2 + W^2 <= 2^31 - 2``).

    TIES: among all sites at the minimum squared distance, the one with the smallest linear index.  With ``spacing`` the passes run
    on float32 maps as in ``distance_transform``: the returned site is a nearest one up to that rounding, and the smallest-index rule
    holds bit for bit wherever the squared distances are exact in float32.

    ``return_distance=True`` returns ``(index, squared_distance)``; the second tensor has the dtype and the bits of
    ``distance_transform(..., squared=True)`` on the same arguments.  ``out``: an int32 tensor of ``labels.shape`` on its device that
    receives the index map (and is returned).

    The call is stream-ordered and reads nothing back.  Contiguous CUDA inputs are read where they lie; other strides are copied first.
    The result is a function of the input alone: the same bits on every run.  The limits raise ``ValueError`` before anything is
    launched; empty inputs return without a launch."""
    what = "nearest_site"
    M.check_labels(what, "labels", labels)
    _, B, D, H, W = M.extent(what, "labels", labels, dims, squares=True)
    background = M.check_int(what, "background", background, allow_none=True)
    foreground = M.check_int(what, "foreground", foreground, allow_none=True)
    if foreground is None and background is None:
        raise ValueError(f"{what}: background=None needs foreground= (there would be no site to measure to)")
    sites_equal = foreground is None
    value = background if sites_equal else foreground
    sp = M.spacing(what, spacing, dims)
    return_distance = bool(return_distance)
    sq_dtype = torch.int32 if sp is None else torch.float32
    dev = labels.device
    M.check_out(what, out, torch.int32, labels)
    sq = None
    if B * D * H * W == 0:
        index = out if out is not None else torch.empty(labels.shape, dtype=torch.int32, device=dev)
        sq = torch.empty(labels.shape, dtype=sq_dtype, device=dev)
    elif not labels.is_cuda:
        sites = _sites_host(labels.contiguous(), B, D, H, W, sites_equal, value if M.fits(value, labels.dtype) else None)
        d, feat = _feature_host(sites, sp)
        index = torch.from_numpy(feat.astype(np.int32)).reshape(labels.shape)
        sq = torch.from_numpy(_squared_form(d, sp)).reshape(labels.shape)
    else:
        x = labels.contiguous()
        index = out if M.direct_out(out) else torch.empty(x.shape, dtype=torch.int32, device=dev)
        sq = torch.empty(x.shape, dtype=sq_dtype, device=dev) if return_distance else None
        _native(what, x, dims, B, D, H, W, sites_equal, value, sp, _INDEX | (_SQUARED if return_distance else 0), index=index, squared=sq)
    index = M.finish_out(out, index)
    return (index, sq) if return_distance else index


def expand_labels(markers, distance=None, mask=None, background=0, dims=2, spacing=None, out=None):
    """Grow the labels of ``markers`` into the positions that hold ``background``: every such position takes the value at its nearest
    labelled position -- the ``nearest_site`` rule, ties to the smallest linear index -- of its own stack entry, provided that

    * ``distance is None`` or its Euclidean distance to it is ``<= distance`` (a finite float ``>= 0``; the comparison is ``squared distance
      <= distance * distance``, in integers with unit spacing), and
    * ``mask is None`` or ``mask`` is non-zero there (``bool`` or ``uint8``, ``markers.shape``, the same device);

    otherwise it holds ``background``.  A labelled position keeps its value; an entry without a labelled position is all ``background``.

    ``markers``: an integer tensor (``bool``, ``uint8``, ``int16``, ``int32``, ``int64``) of shape ``[*stack, (D,) H, W]``; the result has its dtype
    and shape.  ``dims`` and ``spacing`` as in ``distance_transform``, with the same limits.  ``out``: a tensor of markers' dtype, shape and
    device that receives the result (and is returned).

    This is ``skimage.segmentation.expand_labels`` with a mask added.  ``distance=None`` -- unlimited -- is this library's default;
    skimage's is 1.  The distance is EUCLIDEAN, not geodesic: a label can cross a gap of unmasked positions and go on behind it.

    The call is stream-ordered and reads nothing back; contiguous CUDA inputs are read where they lie.  The result is a function of
    the inputs alone: the same bits on every run.  The limits raise ``ValueError`` before anything is launched; empty inputs return
    without a launch."""
    what = "expand_labels"
    M.check_labels(what, "markers", markers)
    _, B, D, H, W = M.extent(what, "labels", markers, dims, squares=True)      # (the rank message has always said "labels")
    background = M.check_int(what, "background", background)
    sp = M.spacing(what, spacing, dims)
    if distance is not None:
        if isinstance(distance, (bool, np.bool_)) or not isinstance(distance, (int, float, np.integer, np.floating)):
            raise TypeError(f"{what}: distance must be None or a float, got {distance!r}")
        distance = float(distance)
        if not (math.isfinite(distance) and distance >= 0):
            raise ValueError(f"{what}: distance must be finite and >= 0, got {distance}")
    dev = markers.device
    if mask is not None:
        M.check_like(what, "mask", mask, markers, (torch.bool, torch.uint8))
    M.check_out(what, out, markers.dtype, markers)
    if B * D * H * W == 0:
        return out if out is not None else torch.empty(markers.shape, dtype=markers.dtype, device=dev)
    max_sq = 0.0
    if distance is not None:
        max_sq = distance * distance
        if sp is None:
            max_sq = float(min(math.floor(max_sq), M.INT_INF))
    if not markers.is_cuda:
        x = markers.contiguous()
        fits = M.fits(background, markers.dtype)
        d, feat = _feature_host(_sites_host(x, B, D, H, W, False, background if fits else None), sp)
        a = x.reshape(B, -1).numpy()
        feat = feat.reshape(B, -1)
        ok = feat >= 0
        if distance is not None:
            ok &= _squared_form(d, sp).reshape(B, -1).astype(np.float64) <= max_sq
        if mask is not None:
            ok &= mask.contiguous().reshape(B, -1).numpy() != 0
        if fits:
            near = np.take_along_axis(a, np.maximum(feat, 0), axis=1)
            res = np.where(a != background, a, np.where(ok, near, a.dtype.type(background)))
        else:                                                     # a background the dtype cannot hold: every position is labelled
            res = a.copy()
        res = torch.from_numpy(res).reshape(markers.shape)
    else:
        x = markers.contiguous()
        m = mask.contiguous() if mask is not None else None
        res = out if M.direct_out(out, x) else torch.empty(x.shape, dtype=x.dtype, device=dev)
        _native(what, x, dims, B, D, H, W, False, background, sp, _GATHER | (_MAX_SQ if distance is not None else 0), gather=res, mask=m, max_sq=max_sq)
    return M.finish_out(out, res)
