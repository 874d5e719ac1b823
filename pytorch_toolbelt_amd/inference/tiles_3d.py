"""3-D tiles: ``VolumeSlicer`` (host geometry / split, numpy) and ``VolumeMerger`` (accumulators in MI355X HBM, HIP
kernels) with the reference's API (``pytorch_toolbelt/inference/tiles_3d.py``).

The reference module is only partly functional: ``VolumeSlicer`` stores the *name* of the weight instead of a window
(tiles_3d.py:46), its ``merge`` reads attributes that only the 2-D slicer has (:140-160) and ``VolumeMerger.
accumulate_single`` indexes with a tuple inside a tuple (:191-192).  What works there -- the slicer geometry, ``split``,
``iter_split``, ``target_shape``, ``crop_to_orignal_size``, ``VolumeMerger.integrate_batch`` and ``merge`` -- is
reproduced exactly (pinned by golden vectors); the broken parts implement the evident intent and are listed in
DESIGN.md.
"""
import ctypes
from typing import Any, Iterable, List, Tuple, Union

import numpy as np
import torch

from .. import _native as N
from . import _host
from ._merge_modes import HeldBatches
from .tta_3d import _activation_code, _check_softmax_channels, apply_activation, flip_view, mirror_views

__all__ = ["VolumeSlicer", "VolumeMerger", "resample_volume"]


def _triple(v, what):
    if isinstance(v, (tuple, list)):
        if len(v) != 3:
            raise ValueError()
        return np.array(v, dtype=int)
    return np.array([int(v)] * 3)


class VolumeSlicer:
    """Slice a ``(D, H, W[, C])`` volume into overlapping ``voxel_size`` blocks every ``voxel_step`` voxels.

    The volume is padded symmetrically (extra voxel goes after) so that an integer number of tiles covers it.
    ``crops[i]`` is a 3-tuple of slices into the PADDED volume (what ``VolumeMerger.integrate_batch`` takes);
    ``bbox_crops[i]`` starts ``pad_before`` earlier (as in the reference).  ``weight``: "mean" -> a ones window (the
    reference keeps the string, which its own ``VolumeMerger`` cannot consume), or a ``[d, h, w]`` ndarray."""

    def __init__(self, volume_shape: Tuple[int, int, int], voxel_size: Union[int, Tuple[int, int, int]],
                 voxel_step: Union[int, Tuple[int, int, int]], weight="mean"):
        self.volume_shape = np.array(volume_shape)[:3]
        self.tile_size = _triple(voxel_size, "voxel_size")
        self.tile_step = _triple(voxel_step, "voxel_step")
        if isinstance(weight, str):
            if weight != "mean":
                raise KeyError(weight)
            self.weight = self._mean(tuple(int(s) for s in self.tile_size))
        else:
            self.weight = weight
        for axis in range(3):
            if self.tile_step[axis] < 1 or self.tile_step[axis] > self.tile_size[axis]:
                raise ValueError()
        overlap = self.tile_size - self.tile_step
        self.num_tiles = np.maximum(1, np.ceil((self.volume_shape - overlap) / self.tile_step)).astype(int)
        self.extra_pad = self.tile_step * self.num_tiles - (self.volume_shape - overlap)
        self.pad_before = self.extra_pad // 2
        self.pad_after = self.extra_pad - self.pad_before
        inner = tuple(slice(int(self.pad_before[a]), int(self.pad_before[a] + self.volume_shape[a])) for a in range(3))
        self.orignal_image_roi = inner
        self.orignal_mask_roi = (slice(None),) + inner
        starts = [range(0, int(self.volume_shape[a] + self.extra_pad[a] - self.tile_size[a] + 1), int(self.tile_step[a])) for a in range(3)]
        self.crops, self.bbox_crops = [], []
        for i in starts[0]:
            for j in starts[1]:
                for k in starts[2]:
                    o = (i, j, k)
                    self.crops.append(tuple(slice(o[a], o[a] + int(self.tile_size[a])) for a in range(3)))
                    self.bbox_crops.append(tuple(slice(o[a] - int(self.pad_before[a]), o[a] + int(self.tile_size[a])) for a in range(3)))

    def _padded(self, volume, value):
        if (np.array(volume.shape[:3]) != self.volume_shape).any() or volume.ndim not in (3, 4):
            raise ValueError(f"Volume shape {volume.shape} is not equal to the expected {self.volume_shape}")
        pad = [(int(b), int(a)) for b, a in zip(self.pad_before, self.pad_after)] + [(0, 0)] * (volume.ndim - 3)
        return np.pad(volume, pad, mode="constant", constant_values=value)

    def split(self, volume: np.ndarray, value=0) -> List[np.ndarray]:
        padded = self._padded(volume, value)
        return [padded[roi].copy() for roi in self.crops]

    def iter_split(self, volume, value=0) -> Iterable[Tuple[np.ndarray, Any]]:
        padded = self._padded(volume, value)
        for roi in self.crops:
            yield padded[roi].copy(), roi

    @property
    def target_shape(self):
        return self.volume_shape + self.extra_pad

    def merge(self, tiles: List[np.ndarray], dtype=np.float32):
        """Host blend in float64 (the evident intent of the reference's non-functional method): weighted sum of the
        tiles over the padded volume, eps-clamped normalisation, ``astype(dtype)``, crop to the volume."""
        if len(tiles) != len(self.crops):
            raise ValueError
        extra = tuple(tiles[0].shape[3:])
        total = np.zeros(tuple(int(s) for s in self.target_shape) + extra, dtype=np.float64)
        mass = np.zeros_like(total)
        w = np.asarray(self.weight, dtype=np.float64).reshape(tuple(self.weight.shape) + (1,) * len(extra))
        for tile, roi in zip(tiles, self.crops):
            total[roi] += tile * w
            mass[roi] += w
        mass = np.clip(mass, a_min=np.finfo(mass.dtype).eps, a_max=None)
        return self.crop_to_orignal_size((total / mass).astype(dtype))

    def crop_to_orignal_size(self, volume):
        return volume[self.orignal_image_roi]

    # ------------------------------------------------------------------ device-side split
    def split_device(self, volume: torch.Tensor, indices=None, scale=None, bias=None, value=0, dtype=torch.float32, mirror=None) -> torch.Tensor:
        """Model input for the tiles ``indices`` straight from a volume that already lives in HBM, as one HIP launch per 64 tiles.

        Equals ``np.stack([np.moveaxis(t, -1, 0) if t.ndim == 4 else t[None] for t in self.split(volume, value)])[indices]`` as a
        float32 tensor (optionally ``* scale[c] + bias[c]``), converted to ``dtype`` -- with no padded copy of the volume, no
        per-tile copies and no upload.  ``volume``: CUDA ``[D, H, W]`` or ``[D, H, W, C]`` (C <= 16) of uint8, int16, uint16,
        float16, bfloat16 or float32; ``indices``: None (all tiles), a slice, or a sequence of tile indices; ``scale`` / ``bias``:
        per-channel sequences (both or neither); ``value``: constant border, cast to the volume's dtype first (as ``np.pad``
        does); ``dtype``: torch.float32, torch.float16 or torch.bfloat16 (round to nearest even).  Returns ``[n, C, d, h, w]``.

        ``mirror``: None, or a mirror string of ``tta_3d`` ("d" .. "dhw"): the result is then
        ``mirror_volume_augment(split_device(...), mirror)``, ``[V*n, C, d, h, w]`` chunk-major, written by the same launches (each
        staged chunk is stored once per view).
        """
        N.require_device(volume, "VolumeSlicer.split_device")
        views = (0,) if mirror is None else mirror_views(mirror)
        code = N.VOLUME_DTYPE_CODES.get(volume.dtype)
        if code is None:
            raise NotImplementedError(f"split_device takes a uint8, int16, uint16, float16, bfloat16 or float32 volume, got {volume.dtype}")
        out_code = N.DTYPE_CODES.get(dtype)
        if out_code is None:
            raise NotImplementedError(f"split_device writes float32, float16 or bfloat16, not {dtype}")
        if volume.dim() not in (3, 4) or tuple(volume.shape[:3]) != tuple(int(s) for s in self.volume_shape):
            raise ValueError(f"Volume shape {tuple(volume.shape)} is not equal to the expected {tuple(int(s) for s in self.volume_shape)}")
        channels = 1 if volume.dim() == 3 else int(volume.shape[3])
        if channels < 1 or channels > 16:
            raise NotImplementedError(f"split_device takes at most 16 channels, got {channels}")
        if (scale is None) != (bias is None):
            raise ValueError("scale and bias go together")
        if indices is None:
            boxes = self.bbox_crops
        elif isinstance(indices, slice):
            boxes = self.bbox_crops[indices]
        else:
            boxes = [self.bbox_crops[int(i)] for i in np.asarray(indices, dtype=np.int64).reshape(-1)]
        d, h, w = (int(s) for s in self.tile_size)
        n = len(boxes)
        out = torch.empty((len(views) * n, channels, d, h, w), device=volume.device, dtype=dtype)
        if n == 0:
            return out
        starts = np.ascontiguousarray(np.array([[s.start for s in box] for box in boxes], dtype=np.int64).T)
        # np.pad assigns the border value into an array of the volume's dtype (the host copy of a bfloat16 volume is float32)
        host_dtype = np.float32 if volume.dtype == torch.bfloat16 else torch.empty(0, dtype=volume.dtype).numpy().dtype
        pad = float(np.asarray(value).astype(host_dtype))
        fa = None
        if scale is not None:
            sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float32).reshape(-1), (channels,)))
            bi = np.ascontiguousarray(np.broadcast_to(np.asarray(bias, dtype=np.float32).reshape(-1), (channels,)))
            fa = (sc.ctypes.data_as(N._fp), bi.ctypes.data_as(N._fp))
        volume = volume.contiguous()
        D, H, W = (int(s) for s in self.volume_shape)
        args = (volume.data_ptr(), code, D, H, W, channels, starts[0].ctypes.data_as(N._i64p), starts[1].ctypes.data_as(N._i64p),
                starts[2].ctypes.data_as(N._i64p), n, d, h, w, fa[0] if fa else None, fa[1] if fa else None, pad)
        if mirror is None:
            N.launch("ptb_volume_split", volume.device, *args, out_code, out.data_ptr(), what="VolumeSlicer.split_device")
        else:
            N.launch("ptb_volume_split_mirror", volume.device, *args, len(views), N.int_array(views), out_code, out.data_ptr(),
                     what="VolumeSlicer.split_device")
        return out

    def _mean(self, volume_size):
        return np.ones(volume_size, dtype=np.float32)


def _resample_size(size, what):
    """``size`` of a resampling call -> three positive ints."""
    try:
        triple = tuple(size)
        ok = len(triple) == 3 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v >= 1 for v in triple)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"{what}: size must be three positive ints (depth, height, width), got {size!r}")
    return tuple(int(v) for v in triple)


def resample_volume(volume: torch.Tensor, size, align_corners: bool = False, dtype=torch.float32) -> torch.Tensor:
    """Trilinear resampling of a ``[D, H, W]`` or ``[D, H, W, C]`` volume to ``size = (D', H', W')`` -- to the spacing the model was trained
    at, before ``VolumeSlicer.split_device`` tiles it.

    Equals ``F.interpolate(volume.float() moved to [1, C, D, H, W], size=size, mode="trilinear", align_corners=align_corners)`` moved back
    to channels last, ``.to(dtype)``.  ``volume``: uint8, int16, uint16, float16, bfloat16 or float32 (what ``split_device`` takes), C <= 16;
    ``dtype``: torch.float32, torch.float16 or torch.bfloat16 (round to nearest even).  A CUDA volume is one HIP launch that widens on load
    and writes the result once (no float32 copy of the input); a CPU volume evaluates the torch expression.  Inference only.  Strong
    down-sampling (a factor of about 4 and more) of a CUDA volume of more than 2^32 - 1 elements raises ``NotImplementedError``."""
    if volume.dtype not in N.VOLUME_DTYPE_CODES:
        raise NotImplementedError(f"resample_volume takes a uint8, int16, uint16, float16, bfloat16 or float32 volume, got {volume.dtype}")
    if dtype not in N.DTYPE_CODES:
        raise NotImplementedError(f"resample_volume writes float32, float16 or bfloat16, not {dtype}")
    if volume.dim() not in (3, 4) or volume.numel() == 0:
        raise ValueError(f"resample_volume takes a non-empty [D, H, W] or [D, H, W, C] volume, got shape {tuple(volume.shape)}")
    size = _resample_size(size, "resample_volume")
    channels = 1 if volume.dim() == 3 else int(volume.shape[3])
    if channels > 16:
        raise NotImplementedError(f"resample_volume takes at most 16 channels, got {channels}")
    if not volume.is_cuda:
        x = volume.float()
        x = x[None, None] if volume.dim() == 3 else x.permute(3, 0, 1, 2)[None]
        y = torch.nn.functional.interpolate(x, size=size, mode="trilinear", align_corners=align_corners)[0]
        return (y[0] if volume.dim() == 3 else y.permute(1, 2, 3, 0)).to(dtype).contiguous()
    if volume.requires_grad:
        raise RuntimeError("resample_volume: the volume requires grad; the HIP resampling is inference-only (use torch.no_grad() / .detach())")
    volume = volume.contiguous()
    out = torch.empty(size + tuple(volume.shape[3:]), device=volume.device, dtype=dtype)
    D, H, W = (int(s) for s in volume.shape[:3])
    N.launch("ptb_volume_resize_trilinear", volume.device, volume.data_ptr(), N.VOLUME_DTYPE_CODES[volume.dtype], D, H, W, channels, *size,
             1 if align_corners else 0, N.DTYPE_CODES[dtype], out.data_ptr(), what="resample_volume")
    return out


def _crop_kind(dtype, argmax):
    """(PTB_CROP_* kind, output dtype) of a 3-D ``merge_crop``."""
    kind = N.CROP_KINDS.get((bool(argmax), dtype))
    if kind is None:
        raise NotImplementedError(f"merge_crop: argmax dtype {dtype} is not supported" if argmax else f"merge_crop: dtype {dtype} is not supported")
    return kind


def _crop_window(crop, shape, layout):
    """``crop`` (a VolumeSlicer: its ``orignal_image_roi``, or ``(z0, y0, x0, D, H, W)``) -> the window, checked against the
    accumulator's ``(D', H', W')``."""
    if isinstance(crop, VolumeSlicer):
        roi = crop.orignal_image_roi
        window = tuple(int(s.start) for s in roi) + tuple(int(s.stop - s.start) for s in roi)
    else:
        window = tuple(int(v) for v in crop)
        if len(window) != 6:
            raise ValueError("a crop window is (z0, y0, x0, depth, height, width)")
    if layout not in ("cdhw", "dhwc"):
        raise ValueError(f"layout must be 'cdhw' or 'dhwc', got {layout!r}")
    for a in range(3):
        if window[a] < 0 or window[3 + a] < 0 or window[a] + window[3 + a] > shape[a]:
            raise ValueError("crop window is outside the accumulator")
    return window


def _roi_starts(rois, tile):
    """``rois``: sequence of 3-tuples of slices (or of ints = starts) -> int64 [3, B] origins; sizes must equal the tile."""
    starts = np.empty((3, len(rois)), dtype=np.int64)
    for b, roi in enumerate(rois):
        if len(roi) != 3:
            raise ValueError("a roi is a (depth, rows, cols) triple")
        for a, s in enumerate(roi):
            if isinstance(s, slice):
                if s.step not in (None, 1) or s.start is None or s.stop is None or s.stop - s.start != tile[a]:
                    raise RuntimeError(f"roi {roi} does not match the tile size {tuple(tile)}")
                starts[a, b] = s.start
            else:
                starts[a, b] = int(s)
    return np.ascontiguousarray(starts)


# ------------------------------------------------------------------------------------------------ deferred slab merge
_DEFER_HINT = "construct the merger without defer=True"
_RESULT_KEYS = ("crop", "layout", "dtype", "argmax")


class _ResultSpec:
    """What a deferred merger writes: the arguments of ``merge_crop`` (``result=dict(crop=, layout=, dtype=, argmax=)``), or with
    ``result=None`` the full padded float32 ``[C, D', H', W']`` volume that ``merge()`` returns."""

    def __init__(self, result, shape):
        self.default = result is None
        result = dict(result or {})
        unknown = sorted(set(result) - set(_RESULT_KEYS))
        if unknown:
            raise ValueError(f"result= takes the arguments of merge_crop {_RESULT_KEYS}, got {unknown}")
        self.layout = result.get("layout", "cdhw")
        self.window = _crop_window(result.get("crop", (0, 0, 0) + tuple(shape)), shape, self.layout)
        self.dtype = result.get("dtype", torch.float32)
        self.argmax = bool(result.get("argmax", False))
        self.kind, self.out_dtype = _crop_kind(self.dtype, self.argmax)

    def out_shape(self, channels):
        od, oh, ow = self.window[3:]
        if self.argmax:
            return (od, oh, ow)
        return (channels, od, oh, ow) if self.layout == "cdhw" else (od, oh, ow, channels)

    def __repr__(self):
        return f"result=dict(crop={self.window}, layout={self.layout!r}, dtype={self.dtype}, argmax={self.argmax})"


class VolumePlan:
    """Host-side plan of a deferred slab merge (``ptb_volume_plan_*``; needs the library, not a GPU): the crop list cut into cells of
    constant covering-tile lists, slabs, launch groups and work items.  ``items()`` is the host-readable table ``[n_items, 16]`` int64:
    launch group, z0, z1, y0, y1, x0, x1 of the box (padded-volume coordinates, inside the window), number of covering tiles, their 8
    indices in integration order (-1 beyond).  ``group_info`` ``[n_groups, 4]``: z0, z1 of the slab, completing tile, items."""

    def __init__(self, crops, tile, shape, channels, window=None, layout="cdhw", kind=N.CROP_F32):
        d, h, w = (int(s) for s in tile)
        D, H, W = (int(s) for s in shape)
        self.starts = _roi_starts(crops, (d, h, w))
        n = self.starts.shape[1]
        window = (0, 0, 0, D, H, W) if window is None else tuple(int(v) for v in window)
        lib = N.load()
        self._lib = lib
        self.handle = ctypes.c_void_p()
        nbytes = lib.ptb_volume_plan_create(self.starts[0].ctypes.data_as(N._i64p), self.starts[1].ctypes.data_as(N._i64p),
                                            self.starts[2].ctypes.data_as(N._i64p), n, int(channels), d, h, w, D, H, W, N.i64_array(window),
                                            1 if layout == "dhwc" else 0, int(kind), ctypes.byref(self.handle))
        if nbytes < 0:
            self.handle = None
            if nbytes == N.PTB_EUNSUPPORTED:
                raise NotImplementedError("deferred slab merge: more than 8 tiles cover a voxel (a step below half the tile), or a tile side "
                                          f"exceeds 65535; {_DEFER_HINT}")
            N.check(int(nbytes), "VolumePlan")
        self.table_bytes = int(nbytes)
        self.n_tiles = n
        n_groups, n_slabs, peak, vec = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        n_items = ctypes.c_int64()
        last = np.zeros(n, dtype=np.int64)
        lib.ptb_volume_plan_info(self.handle, ctypes.byref(n_groups), ctypes.byref(n_slabs), ctypes.byref(n_items), last.ctypes.data_as(N._i64p),
                                 None, ctypes.byref(peak), ctypes.byref(vec))
        info = np.zeros((max(1, n_groups.value), 4), dtype=np.int64)
        lib.ptb_volume_plan_info(self.handle, None, None, None, None, info.ctypes.data_as(N._i64p), None, None)
        self.n_groups, self.n_slabs, self.n_items = n_groups.value, n_slabs.value, int(n_items.value)
        self.last_group_of_tile = last
        self.group_info = info[:self.n_groups]
        self.peak_held_tiles = peak.value
        self.vec_ok = bool(vec.value)

    def items(self):
        rows = np.zeros((max(1, self.n_items), 16), dtype=np.int64)
        got = self._lib.ptb_volume_plan_items(self.handle, rows.ctypes.data_as(N._i64p), self.n_items)
        if got < 0:
            N.check(int(got), "VolumePlan.items")
        return rows[:self.n_items]

    def close(self):
        if getattr(self, "handle", None):
            self._lib.ptb_volume_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DeferredVolume:
    """What the HIP and the torch-op merger share in deferred mode: the planned sequence, the image's configuration, the result spec."""

    _defer = None

    def _defer_setup(self, crops, defer, result, shape, tile):
        if not defer:
            if crops is not None or result is not None:
                raise ValueError(f"{type(self).__name__}: crops= and result= belong to defer=True")
            return False
        if crops is None:
            raise ValueError(f"{type(self).__name__}: defer=True needs crops= (the whole crop sequence, in integration order)")
        self._spec = _ResultSpec(result, shape)
        self._starts = _roi_starts(list(crops), tile)
        if self._starts.shape[1] == 0:
            raise ValueError(f"{type(self).__name__}: crops= is empty")
        self._pos, self._config = 0, None
        self._defer = True
        return True

    def _next_rois(self, rois, what):
        """``rois`` must be the next planned crops; returns their count."""
        tile = tuple(int(s) for s in self.weight.shape[1:])
        starts = _roi_starts(rois, tile)
        n, pos = self._starts.shape[1], self._pos
        if pos + len(rois) > n or not np.array_equal(starts, self._starts[:, pos:pos + len(rois)]):
            raise RuntimeError(f"{what}: the rois are not the next {len(rois)} entries of crops= (tile {pos} of {n} is due); a deferred merger takes "
                               f"the planned sequence in order -- {_DEFER_HINT}")
        return len(rois)

    def _same_config(self, config, what):
        if self._pos == 0:
            self._config = config
        elif config != self._config:
            raise RuntimeError(f"{what}: dtype / mirror / reduction / layout / activation {config} differ from the image's first batch {self._config}; one configuration "
                               f"per image in deferred mode -- {_DEFER_HINT}")

    def _finished_result(self, what):
        n = self._starts.shape[1]
        if self._pos != n:
            raise RuntimeError(f"{what}: only {self._pos} of the {n} planned tiles are in; a deferred merger has no accumulators to read early -- "
                               f"{_DEFER_HINT}")
        return self._result

    def _deferred_merge(self):
        if not self._spec.default:
            raise ValueError(f"merge(): this deferred merger writes {self._spec!r}; call merge_crop with these arguments, or {_DEFER_HINT}")
        out = self._finished_result("VolumeMerger.merge")
        return out if self.dtype == out.dtype else out.to(self.dtype)

    def _deferred_merge_crop(self, crop, layout, dtype, argmax):
        spec = self._spec
        shape = tuple(int(s) for s in self._volume_shape)
        window = _crop_window(crop, shape, layout)
        kind, _ = _crop_kind(dtype, argmax)
        if window != spec.window or layout != spec.layout or kind != spec.kind:
            raise ValueError(f"merge_crop(crop={window}, layout={layout!r}, dtype={dtype}, argmax={argmax}): this deferred merger writes {spec!r}; "
                             f"call it with these arguments, or {_DEFER_HINT}")
        return self._finished_result("VolumeMerger.merge_crop")

    def _no_accumulators(self, name):
        raise RuntimeError(f"VolumeMerger.{name}: a deferred merger keeps no accumulators (the slabs write the result directly) -- {_DEFER_HINT}")


class VolumeMerger(_DeferredVolume):
    """Blend 3-D tile predictions into a full volume that lives in HBM (reference inference/tiles_3d.py:169-211).

    ``volume`` ``[C, D, H, W]``, ``norm_mask`` ``[1, D, H, W]`` and ``weight`` ``[1, d, h, w]`` are public fp32 tensors
    on the GPU.  ``integrate_batch`` adds ``tile * weight`` tile after tile (bit-identical to the reference's loop).  A model output
    in ``torch.channels_last_3d`` (float32 / float16 / bfloat16, on the merger's device) is read where it lies by ``integrate_batch``,
    ``integrate_batch_deaugment`` and ``accumulate_single`` -- no dense or float32 copy, the same bits.

    ``crops=, defer=True[, result=]`` (keyword-only, opt-in): the deferred slab merge.  The merger keeps references to the model
    outputs instead of accumulating them; when the last tile over a z-slab of the plan is in, one launch reads every covering tile,
    blends in integration order in registers and writes ``sum / norm`` straight into the result -- bit for bit what the plain
    ``integrate_batch`` / ``integrate_batch_deaugment`` calls followed by ``merge_crop(**result)`` (``result=None``: ``merge()``)
    give, with no ``volume`` / ``norm_mask`` in memory.  ``result``: the arguments of ``merge_crop`` as a dict (``crop``, ``layout``,
    ``dtype``, ``argmax``); ``merge_crop`` called with the same arguments returns the tensor the slabs wrote.  The contract is
    strict: ``rois`` must be the next entries of ``crops``; batches are CUDA float32 / float16 / bfloat16 on the merger's device, read
    as they are (dense or ``torch.channels_last_3d``: the caller's tensor itself is held; other strides are copied), and must stay alive and unmodified until their slabs are merged (``_merge_modes.HeldBatches``); dtype / mirror /
    reduction / layout are fixed by an image's first batch; ``merge`` / ``merge_crop`` come after the last tile; ``volume`` / ``norm_mask``
    do not exist.  Anything else raises and says to construct the merger without ``defer=True``.  The price of the mode is custody:
    ``peak_held_tiles`` (from the plan) is the most tiles held at once -- with z-major crops two z-layers of tiles, plus the batch in
    flight (98 tiles = 3.3 GB for 343 tiles of 4 x 128^3 float32; 8 x that with the 8 float32 views of ``"dhw"``).  No byte budget is
    enforced.  More than 8 tiles over a voxel (a step below half the tile) raises ``NotImplementedError``.  ``reset()`` starts the
    next volume of the same geometry on the same plan.

    ``activation=, temperature=`` (keyword-only, on ``integrate_batch``, ``accumulate_single`` and ``integrate_batch_deaugment``, plain and
    deferred): the call means the same call on ``A(batch) = (batch.float() * temperature).sigmoid()`` / ``.softmax(dim=1)`` -- the
    reference's ``ApplySigmoidTo`` / ``ApplySoftmaxTo`` -- evaluated inside the merge launch on the logits where they lie
    (``ptb_volume_activation.hip``; dense or ``channels_last_3d``, float32 / float16 / bfloat16), so no probability tensor is written.  The
    source then counts as float32: the reduced value of a half-precision batch is not rounded to the batch's dtype.  Softmax serves
    1 <= C <= 16 (NotImplementedError above; apply ``y.softmax(1)`` yourself), sigmoid any C.  A deferred merger holds the caller's raw
    logits, and activation and temperature belong to the image's configuration.  ``activation=None`` is the call without the keyword."""

    def __new__(cls, volume_shape=None, channels=None, weight=None, device="cpu", *args, **kwargs):
        # like TileMerger: the device the caller names decides -- "cpu" (the reference's default) and float64 accumulators are the
        # torch-op merger, "cuda" the HIP one
        if cls is VolumeMerger:
            dtype = kwargs.get("dtype", args[0] if args else torch.float32)
            from .tiles import _torch_op_accumulators      # (float64 always; float16 / bfloat16 under tiles.set_reference_accumulators(True))

            if torch.device(device).type != "cuda" or _torch_op_accumulators(dtype):
                return object.__new__(HostBackedVolumeMerger)
        return object.__new__(cls)

    def __init__(self, volume_shape, channels: int, weight, device="cpu", dtype=torch.float32, *, crops=None, defer=False, result=None):
        from .tiles import _resolve_device

        device = _resolve_device(device, "VolumeMerger")
        if dtype not in (torch.float32, torch.float16, torch.bfloat16, torch.float64):
            raise TypeError(f"VolumeMerger: dtype must be a floating point type, got {dtype}")
        from .tiles import _torch_op_accumulators

        if _torch_op_accumulators(dtype):  # (VolumeMerger(...) itself routes these to the torch-op merger in __new__; a subclass would sum in float32)
            raise TypeError(f"{type(self).__name__}: {str(dtype).replace('torch.', '')} accumulators are kept by the torch-op merger (VolumeMerger(..., dtype={dtype}) / "
                            "HostBackedVolumeMerger); the HIP kernels of this class accumulate in float32")
        self.dtype = dtype          # honoured by merge(); the accumulators themselves are float32 (see TileMerger)
        dtype = torch.float32
        N.load()
        self.channels = channels
        shape = tuple(int(s) for s in volume_shape)
        self.weight = torch.from_numpy(np.expand_dims(np.asarray(weight), axis=0)).to(device=device, dtype=dtype).contiguous()
        self._volume_shape = shape
        if self._defer_setup(crops, defer, result, shape, tuple(int(s) for s in self.weight.shape[1:])):
            spec = self._spec
            self._plan = VolumePlan(list(crops), self.weight.shape[1:], shape, channels, spec.window, spec.layout, spec.kind)
            self.peak_held_tiles = self._plan.peak_held_tiles
            self._held = HeldBatches("VolumeMerger")
            self._groups_done = 0
            self._table = torch.empty(max(16, self._plan.table_bytes), device=device, dtype=torch.uint8)   # the library allocates no device memory
            N.launch("ptb_volume_plan_upload", self._table.device, self._plan.handle, self._table.data_ptr(), what="VolumeMerger", count=False)
            self._result = torch.empty(spec.out_shape(channels), device=device, dtype=spec.out_dtype)
            return
        self.volume = torch.zeros((channels, *shape), device=device, dtype=dtype)
        self.norm_mask = torch.zeros((1, *shape), device=device, dtype=dtype)

    # ``volume`` / ``norm_mask``: plain attributes of a plain merger; a deferred one has none to show
    @property
    def volume(self):
        if self._defer:
            self._no_accumulators("volume")
        return self._volume

    @volume.setter
    def volume(self, value):
        self._volume = value

    @property
    def norm_mask(self):
        if self._defer:
            self._no_accumulators("norm_mask")
        return self._norm_mask

    @norm_mask.setter
    def norm_mask(self, value):
        self._norm_mask = value

    def reset(self):
        """Start the next volume of the same geometry: a plain merger zeroes ``volume`` and ``norm_mask``; a deferred one keeps its plan
        and device table and gets a fresh result tensor (the caller may still hold the previous one)."""
        if not self._defer:
            self.volume.zero_()
            self.norm_mask.zero_()
            return
        N.check(N.load().ptb_volume_plan_reset(self._plan.handle), "VolumeMerger.reset")
        self._held.clear()
        self._pos, self._config, self._groups_done = 0, None, 0
        self._result = torch.empty(self._spec.out_shape(self.channels), device=self.weight.device, dtype=self._spec.out_dtype)

    def _submit(self, batch, rois, views, code, what, act=N.ACT_NONE, temperature=1.0):
        """Deferred mode: take the batch into custody and launch every slab that is now complete."""
        if not torch.is_tensor(batch) or not batch.is_cuda:
            raise RuntimeError(f"{what}: a deferred merger reads the batches where they lie, on the GPU -- got a host batch; move it to "
                               f"{self.weight.device}, or {_DEFER_HINT}")
        if batch.requires_grad:
            raise RuntimeError(f"{what}: the batch requires grad; a deferred merger holds inference outputs (use torch.no_grad() / "
                               f".detach()), or {_DEFER_HINT}")
        if batch.device != self.weight.device:
            raise ValueError(f"{what}: batch is on {batch.device}, the merger on {self.weight.device}")
        dtype = N.DTYPE_CODES.get(batch.dtype)
        if dtype is None:
            raise NotImplementedError(f"{what} takes float32, float16 or bfloat16 batches, got {batch.dtype}")
        d, h, w = (int(s) for s in self.weight.shape[1:])
        if tuple(batch.shape[1:]) != (self.channels, d, h, w):
            raise RuntimeError(f"tile batch of shape {tuple(batch.shape)} does not match [{'V*' if views else ''}B, {self.channels}, {d}, {h}, {w}]")
        B = self._next_rois(rois, what)
        # a channels_last_3d model output is held and read where it lies (N.SRC_CHANNELS_LAST); any other strides are copied
        layout = N.volume_layout(batch)
        channels_last = layout == N.LAYOUT_CHANNELS_LAST
        config = (batch.dtype, tuple(views), code, "channels_last_3d" if channels_last else "dense")
        if act != N.ACT_NONE:
            _check_softmax_channels(act, self.channels, what)
            config += (act, temperature)
        self._same_config(config, what)
        if B == 0:
            return
        if layout == N.LAYOUT_OTHER:
            batch = batch.contiguous()          # (the copy is what is held)
        if channels_last:
            dtype |= N.SRC_CHANNELS_LAST
        plan, pos = self._plan, self._pos
        due = self._groups_done < plan.n_groups and int(plan.group_info[self._groups_done, 2]) < pos + B
        span = self._held.admit(batch, due)
        tile_elems = self.channels * d * h * w
        dev = self.weight.device
        args = (plan.handle, pos, B, batch.data_ptr(), tile_elems, B * tile_elems, dtype, len(views), N.int_array(views) if views else None, code,
                self.weight.data_ptr(), self._result.data_ptr())
        if act == N.ACT_NONE:
            rc = N.launch("ptb_volume_plan_submit", dev, *args, raw=True)
        else:
            rc = N.launch("ptb_volume_plan_submit_act", dev, *args, act, temperature, raw=True)
        if rc < 0:
            N.check(rc, what)
        self._held.keep(batch, span, last_group=int(plan.last_group_of_tile[pos:pos + B].max()))
        self._pos = pos + B
        self._groups_done += rc
        self._held.rows = [row for row in self._held.rows if row[2] >= self._groups_done]   # the last launch that reads them is out

    def _check_accumulators(self, what):
        for t in (self.volume, self.norm_mask, self.weight):
            N.require_device(t, what)
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("VolumeMerger accumulators must be contiguous float32 tensors")

    def _accumulate(self, batch, rois):
        self._check_accumulators("VolumeMerger")
        d, h, w = (int(s) for s in self.weight.shape[1:])
        if tuple(batch.shape[1:]) != (self.channels, d, h, w):
            raise RuntimeError(f"tile batch of shape {tuple(batch.shape)} does not match [B, {self.channels}, {d}, {h}, {w}]")
        starts = _roi_starts(rois, (d, h, w))
        D, H, W = (int(s) for s in self.volume.shape[1:])
        dev = self.volume.device
        N.launch("ptb_volume_accumulate", dev, self.volume.data_ptr(), self.norm_mask.data_ptr(), self.weight.data_ptr(), batch.data_ptr(),
                 starts[0].ctypes.data_as(N._i64p), starts[1].ctypes.data_as(N._i64p), starts[2].ctypes.data_as(N._i64p), len(rois), self.channels,
                 d, h, w, D, H, W, what="VolumeMerger.integrate_batch")

    def accumulate_single(self, tile: torch.Tensor, roi, *, activation=None, temperature=1.0):
        """Accumulate one ``[C, d, h, w]`` prediction at ``roi`` (3 slices); ``activation`` / ``temperature``: see the class."""
        if _activation_code(activation, temperature, "VolumeMerger.accumulate_single") != N.ACT_NONE:
            return self.integrate_batch(tile.unsqueeze(0), [roi], activation=activation, temperature=temperature)
        if self._defer:
            return self.integrate_batch(tile.unsqueeze(0), [roi])
        if self._channels_last(tile.unsqueeze(0)):
            return self.integrate_batch(tile.unsqueeze(0), [roi])
        self._accumulate(tile.detach().to(device=self.volume.device, dtype=torch.float32).unsqueeze(0).contiguous(), [roi])

    def integrate_batch(self, batch: torch.Tensor, rois, *, activation=None, temperature=1.0):
        """Accumulate ``[B, C, d, h, w]`` predictions at ``rois[b]`` (3 slices each); ``activation`` / ``temperature``: see the class (a host
        batch is uploaded as without them, in its own dtype, and then activated in the launch)."""
        if len(batch) != len(rois):
            raise ValueError("Number of images in batch does not correspond to number of coordinates")
        act = _activation_code(activation, temperature, "VolumeMerger.integrate_batch")
        if act != N.ACT_NONE:
            if self._defer:
                return self._submit(batch, rois, (), 0, "VolumeMerger.integrate_batch", act, float(temperature))
            batch = batch.detach().to(device=self.volume.device)
            if batch.dtype not in N.DTYPE_CODES:
                batch = batch.float()
            return self._mirror_accumulate(batch, rois, (0,), N.RED_SUM, "VolumeMerger.integrate_batch", act, float(temperature))
        if self._defer:
            return self._submit(batch, rois, (), 0, "VolumeMerger.integrate_batch")
        if self._channels_last(batch):       # read where it lies: the identity view summed (exact), so no float32 / dense copy exists
            return self._mirror_accumulate(batch.detach(), rois, (0,), N.RED_SUM, "VolumeMerger.integrate_batch")
        self._accumulate(batch.detach().to(device=self.volume.device, dtype=torch.float32).contiguous(), rois)

    def _channels_last(self, batch):
        """The batch is a channels_last_3d model output the kernels of ptb_volume_channels_last.hip read as it is."""
        return (torch.is_tensor(batch) and batch.is_cuda and batch.device == self.volume.device and batch.dtype in N.DTYPE_CODES
                and N.volume_layout(batch) == N.LAYOUT_CHANNELS_LAST)

    def _mirror_accumulate(self, batch, rois, views, code, what, act=N.ACT_NONE, temperature=1.0):
        """``ptb_volume_mirror_accumulate`` (with an activation: ``ptb_volume_mirror_accumulate_act``) on a dense or channels_last_3d
        ``[V*B, C, d, h, w]`` batch of the accumulators' device."""
        self._check_accumulators("VolumeMerger")
        dtype = N.DTYPE_CODES[batch.dtype]
        d, h, w = (int(s) for s in self.weight.shape[1:])
        if tuple(batch.shape[1:]) != (self.channels, d, h, w):
            raise RuntimeError(f"tile batch of shape {tuple(batch.shape)} does not match [{'V*' if len(views) > 1 else ''}B, {self.channels}, {d}, {h}, {w}]")
        _check_softmax_channels(act, self.channels, what)
        if N.volume_layout(batch) == N.LAYOUT_CHANNELS_LAST:
            dtype |= N.SRC_CHANNELS_LAST
        else:
            batch = batch.contiguous()
        starts = _roi_starts(rois, (d, h, w))
        D, H, W = (int(s) for s in self.volume.shape[1:])
        dev = self.volume.device
        args = (self.volume.data_ptr(), self.norm_mask.data_ptr(), self.weight.data_ptr(), batch.data_ptr(), dtype, len(views), N.int_array(views),
                code, starts[0].ctypes.data_as(N._i64p), starts[1].ctypes.data_as(N._i64p), starts[2].ctypes.data_as(N._i64p), len(rois),
                self.channels, d, h, w, D, H, W)
        if act == N.ACT_NONE:
            N.launch("ptb_volume_mirror_accumulate", dev, *args, what=what)
        else:
            N.launch("ptb_volume_mirror_accumulate_act", dev, *args, act, temperature, what=what)

    def integrate_batch_deaugment(self, batch: torch.Tensor, rois, mirror: str = "dhw", reduction="mean", *, activation=None, temperature=1.0):
        """Fused ``integrate_batch(mirror_volume_deaugment(batch, mirror, reduction), rois)``, bit for bit -- with ``activation`` /
        ``temperature`` (see the class) of ``integrate_batch(mirror_volume_deaugment(batch, mirror, reduction, activation=, temperature=), rois)``.

        ``batch``: the model output for the ``mirror_volume_augment``-ed tiles, ``[V*B, C, d, h, w]`` chunk-major, float32, float16 or
        bfloat16, on the merger's CUDA device (read as it is, no float32 copy; unlike ``integrate_batch``, a host batch is refused
        rather than uploaded -- de-augment it with ``mirror_volume_deaugment`` first).  One launch per tile un-flips the V views, reduces them in fp32 in view
        order (a half-precision result is rounded to the batch's dtype, as ``mirror_volume_deaugment`` returns it) and blends.  A
        reduction that cannot be fused (a callable or None) raises ValueError."""
        from .tta import _reduction_code

        views = mirror_views(mirror)
        if len(batch) != len(views) * len(rois):
            raise ValueError("Number of images in batch does not correspond to number of coordinates x views")
        code = _reduction_code(reduction)
        if code is None:
            raise ValueError(f"reduction={reduction!r} cannot be fused into the tile merge")
        act = _activation_code(activation, temperature, "VolumeMerger.integrate_batch_deaugment")
        temperature = float(temperature)
        if self._defer:
            return self._submit(batch, rois, tuple(views), code, "VolumeMerger.integrate_batch_deaugment", act, temperature)
        self._check_accumulators("VolumeMerger")
        dtype = N.DTYPE_CODES.get(batch.dtype)
        if dtype is None:
            raise NotImplementedError(f"integrate_batch_deaugment takes float32, float16 or bfloat16 batches, got {batch.dtype}")
        N.require_device(batch, "VolumeMerger.integrate_batch_deaugment")
        d, h, w = (int(s) for s in self.weight.shape[1:])
        if tuple(batch.shape[1:]) != (self.channels, d, h, w):
            raise RuntimeError(f"tile batch of shape {tuple(batch.shape)} does not match [V*B, {self.channels}, {d}, {h}, {w}]")
        if batch.device != self.volume.device:
            raise ValueError(f"integrate_batch_deaugment: batch is on {batch.device}, the accumulators on {self.volume.device}")
        self._mirror_accumulate(batch.detach(), rois, views, code, "VolumeMerger.integrate_batch_deaugment", act, temperature)

    def merge(self) -> torch.Tensor:
        """``volume / norm_mask`` as a new tensor (no eps clamp: never-covered voxels are NaN)."""
        if self._defer:
            return self._deferred_merge()
        out = torch.empty_like(self.volume)
        dev = self.volume.device
        N.launch("ptb_merge_div", dev, self.volume.data_ptr(), self.norm_mask.data_ptr(), out.data_ptr(), self.channels, self.norm_mask.numel(),
                 what="VolumeMerger.merge")
        return out if self.dtype == torch.float32 else out.to(self.dtype)

    def merge_crop(self, crop, layout: str = "cdhw", dtype=torch.float32, argmax: bool = False) -> torch.Tensor:
        """``merge()`` + crop + layout + cast in one pass that reads and writes only the cropped window.

        Equals ``merger.merge()[(slice(None),) + window]`` (moved to ``layout``, ``.to(dtype)``) or, with ``argmax=True``, its
        ``.argmax(0)`` -- without the second padded ``[C, D', H', W']`` volume.  ``crop``: a ``VolumeSlicer`` (its
        ``orignal_image_roi``) or ``(z0, y0, x0, D, H, W)``; ``layout``: "cdhw" | "dhwc"; ``dtype``: torch.float32 | float16 |
        bfloat16 (round to nearest even) | uint8 (truncating cast, like ``TileMerger.merge_crop``); with ``argmax=True``: torch.uint8
        or torch.int64 (the default float32 gives int64) class indices ``[D, H, W]``.
        """
        if self._defer:
            return self._deferred_merge_crop(crop, layout, dtype, argmax)
        shape = tuple(int(s) for s in self.volume.shape[1:])
        z0, y0, x0, od, oh, ow = _crop_window(crop, shape, layout)
        kind, out_dtype = _crop_kind(dtype, argmax)
        if argmax:
            out_shape = (od, oh, ow)
        else:
            out_shape = (self.channels, od, oh, ow) if layout == "cdhw" else (od, oh, ow, self.channels)
        for t in (self.volume, self.norm_mask):
            N.require_device(t, "VolumeMerger.merge_crop")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("VolumeMerger accumulators must be contiguous float32 tensors")
        out = torch.empty(out_shape, device=self.volume.device, dtype=out_dtype)
        if out.numel() == 0:
            return out
        dev = self.volume.device
        N.launch("ptb_volume_merge_crop", dev, self.volume.data_ptr(), self.norm_mask.data_ptr(), self.channels, *shape, z0, y0, x0, od, oh, ow,
                 1 if layout == "dhwc" else 0, kind, out.data_ptr(), what="VolumeMerger.merge_crop")
        return out


class HostBackedVolumeMerger(VolumeMerger):
    """``VolumeMerger(device="cpu")`` (and ``dtype=torch.float64`` on any device): the reference's torch-op merger
    (inference/tiles_3d.py:169-211) -- ``volume`` / ``norm_mask`` / ``weight`` in the caller's dtype, tiles blended one after the
    other (``volume[:, roi] += tile * weight``), ``merge()`` without an eps clamp."""

    def __init__(self, volume_shape, channels: int, weight, device="cpu", dtype=torch.float32, *, crops=None, defer=False, result=None):
        self.dtype = dtype
        self.channels = channels
        shape = tuple(int(s) for s in volume_shape)
        self.weight = torch.from_numpy(np.expand_dims(np.asarray(weight), axis=0)).to(device=device, dtype=dtype)
        self.volume = torch.zeros((channels, *shape), device=device, dtype=dtype)
        self.norm_mask = torch.zeros((1, *shape), device=device, dtype=dtype)
        self._volume_shape = shape
        # deferred mode on the host: the same interface and sequence checks; the tiles are blended at once (nothing is held), and the
        # merge_crop expression runs once, when the last tile is in
        if self._defer_setup(crops, defer, result, shape, tuple(int(s) for s in self.weight.shape[1:])):
            self.peak_held_tiles = 0
            self._result = None

    def reset(self):
        self._volume.zero_()
        self._norm_mask.zero_()
        if self._defer:
            self._pos, self._config, self._result = 0, None, None

    def _deferred_blend(self, batch, rois, config, what):
        self._next_rois(rois, what)
        self._same_config(config, what)
        self._blend(batch.to(device=self._volume.device, dtype=self._volume.dtype), rois)
        self._pos += len(rois)
        if self._pos == self._starts.shape[1]:
            spec = self._spec
            self._result = self._host_merge() if spec.default else self._host_merge_crop(spec.window, spec.layout, spec.dtype, spec.argmax)

    @staticmethod
    def _act_config(activation, temperature, what):
        """The activation's part of a deferred image's configuration: () without one."""
        act = _activation_code(activation, temperature, what)
        return () if act == N.ACT_NONE else (act, float(temperature))

    def _blend(self, tiles, rois):
        d, h, w = (int(s) for s in self.weight.shape[1:])
        if tuple(tiles.shape[1:]) != (self.channels, d, h, w):
            raise RuntimeError(f"tile batch of shape {tuple(tiles.shape)} does not match [B, {self.channels}, {d}, {h}, {w}]")
        starts = _roi_starts(rois, (d, h, w))          # (validates the ROIs like the HIP merger: 3 slices of the window's extent)
        D, H, W = (int(s) for s in self._volume.shape[1:])
        for tile, z, y, x in zip(tiles, starts[0], starts[1], starts[2]):
            z, y, x = int(z), int(y), int(x)
            if z < 0 or y < 0 or x < 0 or z + d > D or y + h > H or x + w > W:
                raise RuntimeError("VolumeMerger.integrate_batch: tile rectangle outside the accumulator")
            roi = (slice(None), slice(z, z + d), slice(y, y + h), slice(x, x + w))
            self._volume[roi] += tile * self.weight
            self._norm_mask[roi] += self.weight

    def accumulate_single(self, tile: torch.Tensor, roi, *, activation=None, temperature=1.0):
        if self._defer or _activation_code(activation, temperature, "VolumeMerger.accumulate_single") != N.ACT_NONE:
            return self.integrate_batch(tile.unsqueeze(0), [roi], activation=activation, temperature=temperature)
        self._blend(tile.to(device=self.volume.device, dtype=self.volume.dtype).unsqueeze(0), [roi])

    def integrate_batch(self, batch: torch.Tensor, rois, *, activation=None, temperature=1.0):
        """``VolumeMerger.integrate_batch`` in torch ops; an activation is ``A(batch)`` evaluated first (``tta_3d.apply_activation``)."""
        if len(batch) != len(rois):
            raise ValueError("Number of images in batch does not correspond to number of coordinates")
        act = self._act_config(activation, temperature, "VolumeMerger.integrate_batch")
        if self._defer:
            return self._deferred_blend(apply_activation(batch, activation, temperature), rois, (batch.dtype, (), 0) + act, "VolumeMerger.integrate_batch")
        batch = apply_activation(batch, activation, temperature)
        self._blend(batch.to(device=self.volume.device, dtype=self.volume.dtype), rois)

    def integrate_batch_deaugment(self, batch: torch.Tensor, rois, mirror: str = "dhw", reduction="mean", *, activation=None, temperature=1.0):
        """``VolumeMerger.integrate_batch_deaugment`` in torch ops: the views un-flipped and reduced in the batch's dtype
        (``_host.reduce_stack``; with an activation: of ``A(batch)``, float32), then blended by ``integrate_batch``."""
        from .tta import _reduction_code

        views = mirror_views(mirror)
        if len(batch) != len(views) * len(rois):
            raise ValueError("Number of images in batch does not correspond to number of coordinates x views")
        code = _reduction_code(reduction)
        if code is None:
            raise ValueError(f"reduction={reduction!r} cannot be fused into the tile merge")
        act = self._act_config(activation, temperature, "VolumeMerger.integrate_batch_deaugment")
        raw_dtype = batch.dtype
        batch = apply_activation(batch.to(device=self._volume.device), activation, temperature)
        if N.volume_layout(batch) == N.LAYOUT_CHANNELS_LAST:
            batch = batch.contiguous()      # torch's sum over the stacked views follows the strides: reduce as the dense batch does
        stack = torch.stack([flip_view(c, m) for c, m in zip(torch.chunk(batch, len(views)), views)])
        if self._defer:
            return self._deferred_blend(_host.reduce_stack(stack, code), rois, (raw_dtype, tuple(views), code) + act, "VolumeMerger.integrate_batch_deaugment")
        self.integrate_batch(_host.reduce_stack(stack, code), rois)

    def _host_merge(self):
        return self._volume / self._norm_mask

    def merge(self) -> torch.Tensor:
        if self._defer:
            return self._deferred_merge()
        return self._host_merge()

    def merge_crop(self, crop, layout: str = "cdhw", dtype=torch.float32, argmax: bool = False) -> torch.Tensor:
        """``VolumeMerger.merge_crop`` with torch ops: the cropped window of ``merge()``, moved and converted."""
        if self._defer:
            return self._deferred_merge_crop(crop, layout, dtype, argmax)
        return self._host_merge_crop(crop, layout, dtype, argmax)

    def _host_merge_crop(self, crop, layout, dtype, argmax):
        z0, y0, x0, od, oh, ow = _crop_window(crop, tuple(int(s) for s in self._volume.shape[1:]), layout)
        window = self._host_merge()[:, z0:z0 + od, y0:y0 + oh, x0:x0 + ow]
        _, out_dtype = _crop_kind(dtype, argmax)
        if argmax:
            return window.argmax(dim=0).to(out_dtype)
        out = window.permute(1, 2, 3, 0) if layout == "dhwc" else window
        return out.to(out_dtype).contiguous()
