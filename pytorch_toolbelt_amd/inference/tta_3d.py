"""Mirror test-time augmentation of 3-D volumes (no reference counterpart: the reference has no 3-D TTA).

The spec is the torch expression the functions replace::

    x_aug = torch.cat([x.flip(dims) for dims in FLIPS])                                  # mirror_volume_augment
    y = torch.stack([c.flip(dims) for c, dims in zip(y_aug.chunk(V), FLIPS)]).mean(0)   # mirror_volume_deaugment

A view is a 3-bit mask: bit 0 flips W (dim 4), bit 1 flips H (dim 3), bit 2 flips D (dim 2).  The views of a ``mirror`` string are
every mask made of its axes' bits, in increasing order ("dhw": masks 0..7).  Batches are chunk-major: row ``v * B + b`` holds view
``v`` of tile ``b``.  CUDA tensors run the HIP kernels of ``ptb_volume_tta.hip`` (one launch each); host tensors take the same
expression in torch ops (``_host``), as everywhere in the package.  A ``torch.channels_last_3d`` model output is de-augmented where it
lies (``ptb_volume_channels_last.hip``; fusable reductions), with the bits of its dense copy.  The kernels are inference only: a CUDA tensor that requires grad is
refused with NotImplementedError, while a host tensor keeps torch's autograd through the torch ops.
``VolumeSlicer.split_device(.., mirror=)`` writes the augmented batch straight from the volume and
``VolumeMerger.integrate_batch_deaugment`` un-flips, reduces and blends in one pass per tile.
"""
from typing import Callable, Optional, Tuple, Union

import torch

from .. import _native as N
from . import _host

__all__ = ["MIRROR_VIEWS", "mirror_volume_augment", "mirror_volume_deaugment"]

_AXIS_BITS = {"d": 4, "h": 2, "w": 1}


def _views_of(axes: str) -> Tuple[int, ...]:
    bits = sum(_AXIS_BITS[a] for a in axes)
    return tuple(m for m in range(8) if m & ~bits == 0)


MIRROR_VIEWS = {axes: _views_of(axes) for axes in ("d", "h", "w", "dh", "dw", "hw", "dhw")}


def mirror_views(mirror: str) -> Tuple[int, ...]:
    """The view masks of ``mirror``; anything but the 7 mirror strings raises ValueError."""
    if not isinstance(mirror, str) or mirror not in MIRROR_VIEWS:
        raise ValueError(f"mirror must be one of {', '.join(repr(k) for k in MIRROR_VIEWS)}, got {mirror!r}")
    return MIRROR_VIEWS[mirror]


def flip_view(x: torch.Tensor, mask: int) -> torch.Tensor:
    """View ``mask`` of a ``[B, C, D, H, W]`` tensor (its own inverse)."""
    dims = [dim for dim, bit in ((2, 4), (3, 2), (4, 1)) if mask & bit]
    return x.flip(dims) if dims else x


def _check_volume_batch(x: torch.Tensor, what: str) -> int:
    """Validate a CUDA ``[B, C, D, H, W]`` tensor for the kernels; returns its PTB_* dtype code."""
    N.require_device(x, what)
    if x.dim() != 5:
        raise ValueError(f"{what}: expected a [B, C, D, H, W] tensor, got shape {tuple(x.shape)}")
    code = N.DTYPE_CODES.get(x.dtype)
    if code is None:
        raise NotImplementedError(f"{what} takes float32, float16 or bfloat16 tensors, got {x.dtype}")
    if x.requires_grad:
        raise NotImplementedError(f"{what} is inference only: the tensor requires grad")
    return code


def _divisible(n: int, V: int):
    if n % V != 0:
        raise RuntimeError(f"Input batch size ({n}) must be divisible by {V}.")


def _mirror(x: torch.Tensor, code: int, views, in_is_batch: bool, out_shape) -> torch.Tensor:
    x = x.contiguous()
    n, C, D, H, W = x.shape
    out = torch.empty(out_shape, device=x.device, dtype=x.dtype)
    lib = N.load()
    with N.on_device(x.device):
        rc = lib.ptb_volume_mirror(x.data_ptr(), code, out.data_ptr(), len(views), N.int_array(views), 1 if in_is_batch else 0,
                                   n if in_is_batch else n // len(views), C, D, H, W, N.stream_ptr(x.device))
    N.bump()
    N.check(rc, "ptb_volume_mirror")
    return out


def mirror_volume_augment(x: torch.Tensor, mirror: str = "dhw") -> torch.Tensor:
    """``torch.cat([flip_v(x) for v in views])``: ``[B, C, D, H, W]`` -> ``[V*B, C, D, H, W]``, chunk-major, in one launch."""
    views = mirror_views(mirror)
    if x.device.type != "cuda":
        return torch.cat([flip_view(x, m) for m in views])
    code = _check_volume_batch(x, "mirror_volume_augment")
    return _mirror(x, code, views, True, (len(views) * x.shape[0],) + tuple(x.shape[1:]))


def mirror_volume_deaugment(y: torch.Tensor, mirror: str = "dhw",
                            reduction: Optional[Union[str, Callable]] = "mean") -> torch.Tensor:
    """Undo ``mirror_volume_augment`` on the model output ``[V*B, C, D, H, W]`` and reduce the views.

    ``reduction``: the reductions of ``tta._deaugment_averaging`` -- "mean" | "sum" | "gmean" | "hmean" | "harmonic1p" | "logodd" |
    "log1p" (and their long names) reduce in fp32 in view order in one launch and return ``[B, C, D, H, W]`` in ``y``'s dtype; a
    callable is given the un-flipped ``[V, B, C, D, H, W]`` stack (``reduction(stack, dim=0)``); None returns that stack."""
    from .tta import _reduction_code

    views = mirror_views(mirror)
    V = len(views)
    _divisible(y.size(0), V)
    code = _reduction_code(reduction)
    if code is None and not (callable(reduction) or reduction in {None, "None", "none"}):
        raise KeyError(f"Unsupported reduction mode {reduction}")
    if y.device.type != "cuda":
        if code is not None and N.volume_layout(y) == N.LAYOUT_CHANNELS_LAST:
            y = y.contiguous()      # torch's sum over the stacked views follows the strides (1 ulp with 8 views): reduce as the dense batch does
        stack = torch.stack([flip_view(c, m) for c, m in zip(torch.chunk(y, V), views)])
    else:
        dtype = _check_volume_batch(y, "mirror_volume_deaugment")
        B = y.shape[0] // V
        if code is not None:
            # a channels_last_3d model output is read where it lies (N.SRC_CHANNELS_LAST); any other strides are copied, as ever
            if N.volume_layout(y) == N.LAYOUT_CHANNELS_LAST:
                dtype |= N.SRC_CHANNELS_LAST
            else:
                y = y.contiguous()
            out = torch.empty((B,) + tuple(y.shape[1:]), device=y.device, dtype=y.dtype)
            _, C, D, H, W = y.shape
            lib = N.load()
            with N.on_device(y.device):
                rc = lib.ptb_volume_mirror_reduce(y.data_ptr(), dtype, out.data_ptr(), V, N.int_array(views), code, B, C, D, H, W,
                                                  N.stream_ptr(y.device))
            N.bump()
            N.check(rc, "ptb_volume_mirror_reduce")
            return out
        stack = _mirror(y, dtype, views, False, (V, B) + tuple(y.shape[1:]))
    if code is not None:
        return _host.reduce_stack(stack, code)
    return reduction(stack, dim=0) if callable(reduction) else stack
