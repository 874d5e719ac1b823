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

``activation=`` ("sigmoid" | "softmax", with ``temperature=``) on ``mirror_volume_deaugment`` and on the ``VolumeMerger`` calls applies
``A(y) = (y.float() * temperature).sigmoid()`` / ``.softmax(dim=1)`` -- the reference's ``ApplySigmoidTo`` / ``ApplySoftmaxTo`` -- to the
model's logits inside the same launch (``ptb_volume_activation.hip``): the call means the call without it on ``A(y)``, a float32 tensor that
is never written.
"""
import math

from typing import Callable, Optional, Tuple, Union

import torch

from .. import _native as N
from . import _host

__all__ = ["MIRROR_VIEWS", "mirror_volume_augment", "mirror_volume_deaugment", "apply_activation"]

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


def _activation_code(activation, temperature, what: str) -> int:
    """PTB_ACT_* of ``activation`` (None | "sigmoid" | "softmax"); anything else, or a non-finite ``temperature``, raises ValueError."""
    if activation is not None and not (isinstance(activation, str) and activation in N.ACT_CODES):
        raise ValueError(f"{what}: activation must be None, 'sigmoid' or 'softmax', got {activation!r}")
    try:
        finite = not isinstance(temperature, bool) and math.isfinite(temperature)
    except TypeError:
        finite = False
    if not finite:
        raise ValueError(f"{what}: temperature must be a finite float, got {temperature!r}")
    return N.ACT_CODES[activation]


def apply_activation(y: torch.Tensor, activation, temperature: float = 1.0) -> torch.Tensor:
    """``A(y)`` in torch ops: ``(y.float() * temperature).sigmoid()`` | ``.softmax(dim=1)`` (float32; ``y`` itself for None) -- what the fused
    calls mean, and what the host paths evaluate."""
    code = _activation_code(activation, temperature, "apply_activation")
    if code == N.ACT_NONE:
        return y
    z = y.float() * float(temperature)
    return z.sigmoid() if code == N.ACT_SIGMOID else z.softmax(dim=1)


def _check_softmax_channels(code: int, channels: int, what: str):
    if code == N.ACT_SOFTMAX and channels > N.ACT_MAX_SOFTMAX_CHANNELS:
        raise NotImplementedError(f"{what}: the fused softmax keeps the channels of a voxel in registers and serves 1..{N.ACT_MAX_SOFTMAX_CHANNELS} "
                                  f"of them, got {channels}; apply y.softmax(1) yourself and call without activation=")


def _divisible(n: int, V: int):
    if n % V != 0:
        raise RuntimeError(f"Input batch size ({n}) must be divisible by {V}.")


def _mirror(x: torch.Tensor, code: int, views, in_is_batch: bool, out_shape) -> torch.Tensor:
    x = x.contiguous()
    n, C, D, H, W = x.shape
    out = torch.empty(out_shape, device=x.device, dtype=x.dtype)
    N.launch("ptb_volume_mirror", x.device, x.data_ptr(), code, out.data_ptr(), len(views), N.int_array(views), 1 if in_is_batch else 0,
             n if in_is_batch else n // len(views), C, D, H, W)
    return out


def mirror_volume_augment(x: torch.Tensor, mirror: str = "dhw") -> torch.Tensor:
    """``torch.cat([flip_v(x) for v in views])``: ``[B, C, D, H, W]`` -> ``[V*B, C, D, H, W]``, chunk-major, in one launch."""
    views = mirror_views(mirror)
    if x.device.type != "cuda":
        return torch.cat([flip_view(x, m) for m in views])
    code = _check_volume_batch(x, "mirror_volume_augment")
    return _mirror(x, code, views, True, (len(views) * x.shape[0],) + tuple(x.shape[1:]))


def _deaugment_activated(y, views, code, act, temperature):
    """``ptb_volume_mirror_reduce_act``: the fused reduction over ``A(y)``, dense float32 out."""
    dtype = _check_volume_batch(y, "mirror_volume_deaugment")
    V = len(views)
    B = y.shape[0] // V
    _, C, D, H, W = y.shape
    _check_softmax_channels(act, C, "mirror_volume_deaugment")
    if N.volume_layout(y) == N.LAYOUT_CHANNELS_LAST:
        dtype |= N.SRC_CHANNELS_LAST
    else:
        y = y.contiguous()
    out = torch.empty((B, C, D, H, W), device=y.device, dtype=torch.float32)
    N.launch("ptb_volume_mirror_reduce_act", y.device, y.data_ptr(), dtype, out.data_ptr(), V, N.int_array(views), code, B, C, D, H, W, act,
             temperature)
    return out


def mirror_volume_deaugment(y: torch.Tensor, mirror: str = "dhw",
                            reduction: Optional[Union[str, Callable]] = "mean", *, activation: Optional[str] = None,
                            temperature: float = 1.0) -> torch.Tensor:
    """Undo ``mirror_volume_augment`` on the model output ``[V*B, C, D, H, W]`` and reduce the views.

    ``reduction``: the reductions of ``tta._deaugment_averaging`` -- "mean" | "sum" | "gmean" | "hmean" | "harmonic1p" | "logodd" |
    "log1p" (and their long names) reduce in fp32 in view order in one launch and return ``[B, C, D, H, W]`` in ``y``'s dtype; a
    callable is given the un-flipped ``[V, B, C, D, H, W]`` stack (``reduction(stack, dim=0)``); None returns that stack.

    ``activation``: None | "sigmoid" | "softmax" (anything else: ValueError), ``temperature``: a finite float.  The call then equals
    ``mirror_volume_deaugment(A(y), mirror, reduction)`` with ``A(y) = (y.float() * temperature).sigmoid()`` / ``.softmax(dim=1)``, so the
    result is float32 whatever ``y``'s dtype.  On a CUDA tensor with a fusable reduction ``A`` runs inside the one launch, on the logits where
    they lie (dense or ``channels_last_3d``, float32 / float16 / bfloat16): per voxel and view ``z = x * temperature`` rounded, sigmoid
    ``1 / (1 + exp(-z))`` (exact 0 / 1 when it saturates, never NaN), softmax ``exp(z - max_c z) / sum_c exp(..)`` summed in channel order,
    then the reduction as without it.  Finite logits are the defined inputs.  The fused softmax serves 1 <= C <= 16 (NotImplementedError
    above that), sigmoid any C.  Host tensors, and a callable or None reduction, apply ``A`` with torch ops and go on as without it."""
    from .tta import _reduction_code

    views = mirror_views(mirror)
    V = len(views)
    _divisible(y.size(0), V)
    code = _reduction_code(reduction)
    if code is None and not (callable(reduction) or reduction in {None, "None", "none"}):
        raise KeyError(f"Unsupported reduction mode {reduction}")
    act = _activation_code(activation, temperature, "mirror_volume_deaugment")
    if act != N.ACT_NONE:
        if y.device.type == "cuda" and code is not None:
            return _deaugment_activated(y, views, code, act, float(temperature))
        y = apply_activation(y, activation, temperature)
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
            N.launch("ptb_volume_mirror_reduce", y.device, y.data_ptr(), dtype, out.data_ptr(), V, N.int_array(views), code, B, C, D, H, W)
            return out
        stack = _mirror(y, dtype, views, False, (V, B) + tuple(y.shape[1:]))
    if code is not None:
        return _host.reduce_stack(stack, code)
    return reduction(stack, dim=0) if callable(reduction) else stack
