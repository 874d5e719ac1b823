"""Connected components of label maps, on the device the tensors are on: the step between ``merge_crop(argmax=True)`` and
``rle_encode_device`` / ``confusion_matrix`` that splits a map into blobs so that small ones can be dropped and the rest counted, boxed
and measured.

The reference has no counterpart (it is pure Python and labels nothing), so the names and meanings below are this library's.  Two
neighbouring positions belong to one component iff they hold the same value and that value is not the background: a 4-class map gives
the components of every class in one call.  Components are numbered ``1 .. n`` in row-major order of their first position, the
numbering of ``scipy.ndimage.label``.

CUDA tensors run the HIP kernels of ``csrc/ptb_components.hip`` (a missing kernel is an error, never a silent host computation), CPU
tensors take the numpy form below with the same results -- the device the caller names decides.
"""
import ctypes

import numpy as np
import torch

from .. import _native as N
from . import _maps as M

__all__ = ["connected_components", "component_stats", "remove_small_components"]

MAX_POSITIONS = M.MAX_POSITIONS


# ---------------------------------------------------------------------------------------------------------------- validation
def _geometry(what, labels, connectivity, background, dims):
    """Validated ``(stack, B, D, H, W, full, background)`` of a labelling call."""
    M.check_labels(what, "labels", labels)
    connectivity, full = M.check_connectivity(what, connectivity, dims)
    background = M.check_int(what, "background", background, allow_none=True)
    stack, B, D, H, W = M.extent(what, "labels", labels, dims, note=" (component numbers are int32)")
    if background is not None and not M.fits(background, labels.dtype):
        background = None                                     # a value the dtype cannot hold occurs nowhere
    return stack, B, D, H, W, full, background


def _workspace(lib, what, dims, B, D, H, W, remove):
    label_bytes, remove_bytes = ctypes.c_int64(), ctypes.c_int64()
    N.check(lib.ptb_cc_plan(dims, B, D, H, W, None, None, None, None, ctypes.byref(label_bytes), ctypes.byref(remove_bytes)), what)
    return remove_bytes.value if remove else label_bytes.value


# ---------------------------------------------------------------------------------------------------------------- host form
def _label_entry_host(a, full, background):
    """``(cc int32 [D, H, W], n)`` of one numpy ``[D, H, W]`` entry.  Correct rather than fast: the rows are cut into runs of equal values,
    runs of neighbouring rows that touch (by a face, or with ``full`` also by an edge or a corner) and hold the same value are joined by
    a union-find over runs -- every root hooks to the smaller root it meets, then all pointers jump to their roots, until no joined pair
    differs -- and the roots are numbered in their order, which is the order of the components' first positions."""
    D, H, W = a.shape
    flat = a.reshape(D * H, W)
    change = np.ones(flat.shape, dtype=bool)
    change[:, 1:] = flat[:, 1:] != flat[:, :-1]
    starts = np.flatnonzero(change.reshape(-1))                               # every row begins a run
    ends = np.append(starts[1:], flat.size)
    values = flat.reshape(-1)[starts]
    keep = np.flatnonzero(values != background) if background is not None else np.arange(starts.size)
    val, row = values[keep], starts[keep] // W
    x0, x1 = starts[keep] - row * W, ends[keep] - row * W                     # [x0, x1) of row `row`
    z, y = row // H, row % H
    S = W + 2                                                                 # key of column x of row r: r * S + x + 1
    skey, ekey = row * S + x0 + 1, row * S + x1 + 1
    d = 1 if full else 0
    ei, ej = [], []
    for dz in ((-1, 0) if D > 1 else (0,)):
        for dy in (-1, 0, 1):
            if not (dz < 0 or dy < 0) or (not full and dz != 0 and dy != 0):
                continue
            ok = (y + dy >= 0) & (y + dy < H) & (z + dz >= 0)
            other = (row + dz * H + dy) * S
            lo = np.searchsorted(ekey, other + x0 + 1 - d, side="right")      # the first run that ends behind x0 - d
            hi = np.searchsorted(skey, other + x1 + 1 + d, side="left")       # the first run that starts at or behind x1 + d
            cnt = np.where(ok, np.maximum(hi - lo, 0), 0)
            i = np.repeat(np.arange(val.size), cnt)
            j = lo[i] + np.arange(i.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            same = val[i] == val[j]
            ei.append(i[same])
            ej.append(j[same])
    ei, ej = np.concatenate(ei), np.concatenate(ej)
    lab = np.arange(val.size)
    while True:
        li, lj = lab[ei], lab[ej]
        differ = li != lj
        if not differ.any():
            break
        ei, ej, li, lj = ei[differ], ej[differ], li[differ], lj[differ]
        np.minimum.at(lab, np.maximum(li, lj), np.minimum(li, lj))
        while True:
            jumped = lab[lab]
            if np.array_equal(jumped, lab):
                break
            lab = jumped
    is_root = lab == np.arange(val.size)
    number = np.cumsum(is_root)                                               # 1-based rank of every root
    ids = np.zeros(starts.size, dtype=np.int32)
    ids[keep] = number[lab]
    return np.repeat(ids, ends - starts).reshape(D, H, W), int(is_root.sum())


def _label_host(labels, B, D, H, W, full, background):
    a = labels.reshape(B, D, H, W).numpy()
    cc = np.zeros((B, D, H, W), dtype=np.int32)
    count = np.zeros(B, dtype=np.int64)
    for b in range(B):
        cc[b], count[b] = _label_entry_host(a[b], full, background)
    return cc, count


# ---------------------------------------------------------------------------------------------------------------- public
def connected_components(labels, connectivity=8, background=0, dims=2):
    """``(cc, count)``: the connected components of ``labels``.

    ``labels``: an integer tensor (``bool``, ``uint8``, ``int16``, ``int32``, ``int64``) of shape ``[*stack, H, W]`` (``dims=2``) or
    ``[*stack, D, H, W]`` (``dims=3``); the entries of ``stack`` (any number of leading dimensions, possibly none) are labelled
    independently, all in the same launches.  Two neighbouring positions are in one component iff they hold the same value and that
    value is not ``background``; ``background=None``: every value is foreground, 0 included; a ``background`` the dtype cannot hold
    occurs nowhere.  ``connectivity``: 4 or 8 for ``dims=2``, 6 or 26 for ``dims=3``.

    ``cc``: int32, the input's shape and device; 0 at background, elsewhere ``1 .. n`` within each stack entry, numbered in row-major
    order of each component's first position (the numbering of ``scipy.ndimage.label``).  ``count``: int64 of shape ``stack`` with ``n``
    per entry (on a CUDA tensor -1 would mean that a step cap of the kernels was exceeded: a bug, never a property of the input).

    The call is stream-ordered and reads nothing back.  Contiguous CUDA inputs are read where they lie (no widened, boolean or
    per-class copy); other strides are copied first.  The result is a function of the input alone: the same bits on every run.  More
    than 2^31 - 2 positions per call raise ``ValueError``; empty inputs return without a launch."""
    what = "connected_components"
    stack, B, D, H, W, full, background = _geometry(what, labels, connectivity, background, dims)
    dev = labels.device
    if B * D * H * W == 0:
        return torch.zeros(labels.shape, dtype=torch.int32, device=dev), torch.zeros(stack, dtype=torch.int64, device=dev)
    if not labels.is_cuda:
        cc, count = _label_host(labels.contiguous(), B, D, H, W, full, background)
        return torch.from_numpy(cc).reshape(labels.shape), torch.from_numpy(count).reshape(stack)
    x = labels.contiguous()
    nbytes = _workspace(N.load(), what, dims, B, D, H, W, remove=False)
    cc = torch.empty(x.shape, dtype=torch.int32, device=dev)
    count = torch.empty(stack, dtype=torch.int64, device=dev)
    ws = M.scratch(nbytes, dev)
    N.launch("ptb_cc_label", dev, x.data_ptr(), M.ELEM_BYTES[x.dtype], dims, B, D, H, W, connectivity, int(background is not None), background or 0,
             cc.data_ptr(), count.data_ptr(), ws.data_ptr(), nbytes, what=what)
    return cc, count


def component_stats(cc, count=None, values=None, max_components=None):
    """Area, bounding box and class of every component of ONE entry's ``cc`` map (``[H, W]`` or ``[D, H, W]``; loop over a stack).

    Returns a dict; row ``i`` describes component ``i + 1``: ``"area"`` int64 ``[n]``; ``"bbox"`` int64 ``[n, 2 * dims]``, minima
    inclusive and maxima exclusive, in ``y0, x0, y1, x1`` or ``z0, y0, x0, z1, y1, x1`` order (``dims = cc.dim()``); ``"value"`` ``[n]`` in
    ``values``' dtype, the value ``values`` (the source label map) holds on the component, present only when ``values`` is given.

    ``n = max_components`` when that is given: nothing is read back, rows past the real count have area 0 (and a zero box and value),
    components numbered above it are left out.  Otherwise ``n`` is read from ``count`` (or ``cc.max()`` when ``count`` is None): 8 bytes,
    the call's only D2H read."""
    what = "component_stats"
    if not isinstance(cc, torch.Tensor) or cc.dtype != torch.int32:
        raise TypeError(f"{what}: cc must be the int32 map of connected_components")
    if cc.dim() not in (2, 3) or (isinstance(count, torch.Tensor) and count.dim() > 0):
        raise ValueError(f"{what}: takes one entry ([H, W] or [D, H, W] with a 0-dim count), got cc {tuple(cc.shape)}"
                         f"{'' if count is None or not isinstance(count, torch.Tensor) else f' and count {tuple(count.shape)}'}: "
                         "loop over the entries of a stack")
    dims = cc.dim()
    if values is not None:
        if not isinstance(values, torch.Tensor) or values.dtype not in M.ELEM_BYTES:
            raise TypeError(f"{what}: values must be an integer label tensor (bool, uint8, int16, int32 or int64)")
        if values.shape != cc.shape or values.device != cc.device:
            raise ValueError(f"{what}: values {tuple(values.shape)} on {values.device} does not match cc {tuple(cc.shape)} on {cc.device}")
    if cc.numel() > MAX_POSITIONS:
        raise ValueError(f"{what}: {cc.numel()} positions; at most 2^31 - 2")
    max_components = M.check_int(what, "max_components", max_components, allow_none=True)
    if max_components is not None:
        if max_components < 0:
            raise ValueError(f"{what}: max_components must be >= 0, got {max_components}")
        n = max_components
    elif count is not None:
        n = int(count.item() if isinstance(count, torch.Tensor) else count)
        if n < 0:
            raise ValueError(f"{what}: count is {n}: the labelling failed")
    else:
        n = int(cc.max().item()) if cc.numel() else 0
    n = min(n, MAX_POSITIONS)
    dev = cc.device
    out = {"area": torch.zeros(n, dtype=torch.int64, device=dev), "bbox": torch.zeros((n, 2 * dims), dtype=torch.int64, device=dev)}
    if values is not None:
        out["value"] = torch.zeros(n, dtype=values.dtype, device=dev)
    if n == 0 or cc.numel() == 0:
        return out
    if not cc.is_cuda:
        _stats_host(cc, values, n, out)
        return out
    x = cc.contiguous()
    v = values.contiguous() if values is not None else None
    D = x.shape[0] if dims == 3 else 1
    N.launch("ptb_cc_stats", dev, x.data_ptr(), dims, D, x.shape[-2], x.shape[-1], n, N.ptr(v), M.ELEM_BYTES[v.dtype] if v is not None else 0,
             out["area"].data_ptr(), out["bbox"].data_ptr(), N.ptr(out.get("value")), what=what)
    return out


def _stats_host(cc, values, n, out):
    a = cc.numpy()
    dims = a.ndim
    pos = np.flatnonzero((a.reshape(-1) >= 1) & (a.reshape(-1) <= n))
    row = a.reshape(-1)[pos].astype(np.int64) - 1
    out["area"] += torch.from_numpy(np.bincount(row, minlength=n).astype(np.int64))
    coords = np.unravel_index(pos, a.shape)
    lo = np.full((n, dims), np.iinfo(np.int64).max, dtype=np.int64)
    hi = np.full((n, dims), -1, dtype=np.int64)
    for d in range(dims):
        np.minimum.at(lo[:, d], row, coords[d])
        np.maximum.at(hi[:, d], row, coords[d])
    seen = out["area"].numpy() > 0
    box = np.where(seen[:, None], np.concatenate([lo, hi + 1], axis=1), 0)
    out["bbox"] += torch.from_numpy(box)
    if values is not None:
        val = out["value"].numpy()
        val[row] = values.numpy().reshape(-1)[pos]


def remove_small_components(labels, min_area, connectivity=8, background=0, dims=2, fill=None, out=None):
    """``labels`` with every connected component of fewer than ``min_area`` positions replaced by ``fill``.

    ``labels``, ``connectivity``, ``background``, ``dims`` and stacks as in ``connected_components``.  ``fill`` defaults to ``background``
    and is required when ``background=None``.  ``out``: a tensor like ``labels`` that receives the result; it may be ``labels`` itself.
    Needs no consecutive numbering, so it runs without the scan: no read-back, no synchronisation."""
    what = "remove_small_components"
    stack, B, D, H, W, full, bg = _geometry(what, labels, connectivity, background, dims)
    min_area = M.check_int(what, "min_area", min_area)
    fill = M.check_int(what, "fill", fill, allow_none=True)
    if fill is None:
        if background is None:
            raise ValueError(f"{what}: fill is required with background=None (there is no background to fill with)")
        fill = int(background)
    if not M.fits(fill, labels.dtype):
        raise ValueError(f"{what}: fill {fill} cannot be held by {labels.dtype}")
    M.check_out(what, out, labels.dtype, labels)
    dev = labels.device
    if B * D * H * W == 0:
        return out if out is not None else labels.clone()
    x = labels.contiguous()
    if not labels.is_cuda:
        cc, _ = _label_host(x, B, D, H, W, full, bg)
        res = x.clone().reshape(B, -1)
        for b in range(B):
            flat = cc[b].reshape(-1)
            small = torch.from_numpy((np.bincount(flat)[flat] < min_area) & (flat > 0))
            res[b][small] = fill
        res = res.reshape(labels.shape)
    else:
        nbytes = _workspace(N.load(), what, dims, B, D, H, W, remove=True)
        res = out if out is not None and out.is_contiguous() else torch.empty_like(x)
        ws = M.scratch(nbytes, dev)
        N.launch("ptb_cc_remove_small", dev, x.data_ptr(), M.ELEM_BYTES[x.dtype], dims, B, D, H, W, connectivity, int(bg is not None), bg or 0, min_area,
                 fill, res.data_ptr(), ws.data_ptr(), nbytes, what=what)
    return M.finish_out(out, res)
