"""What the distance-map, hard-mining and soft-clDice losses make of ``(y_pred, y_true, mode)`` before a kernel or a torch op sees them: the
checks of the configuration and the tensors in the one form every path takes.  Private to ``losses``; the region losses (``_region.py``)
keep their own reading, which raises ``RuntimeError`` where this one raises ``ValueError``."""
from typing import NamedTuple, Optional, Tuple

import torch

from . import _kernels as K
from ._region import BINARY_MODE, MULTICLASS_MODE, MULTILABEL_MODE

__all__ = []


def check_mode(what, mode):
    if mode not in (BINARY_MODE, MULTICLASS_MODE, MULTILABEL_MODE):
        raise ValueError(f"{what}: mode must be 'binary', 'multiclass' or 'multilabel', got {mode!r}")


def check_classes(what, mode, classes):
    """``classes=`` of a constructor as a list of ints, or None"""
    if classes is None:
        return None
    if mode == BINARY_MODE:
        raise ValueError(f"{what}: masking classes is not supported with mode='binary'")
    classes = [int(c) for c in classes]
    if not classes or len(set(classes)) != len(classes) or min(classes) < 0:
        raise ValueError(f"{what}: classes must be distinct non-negative ints, got {classes!r}")
    return classes


class Problem(NamedTuple):
    x: torch.Tensor                          # fp32 contiguous [B, C, S]
    labels: Optional[torch.Tensor]           # int64 contiguous [B, S] (multiclass), or None ...
    dense: Optional[torch.Tensor]            # ... and fp32 contiguous [B, C, S]
    prob: int                                # K.PROB_*: the activation the kernels apply
    B: int
    C: int
    spatial: Tuple[int, ...]
    S: int
    ignore: Tuple[bool, int, float]          # (has_ignore, ignore_label, ignore_value)


def problem(what, y_pred, y_true, mode, from_logits, ignore_index=None, dims=None, half_or_single=False, exact_labels=False, detach_target=False):
    """The ``Problem`` of a call.  ``dims=None``: 2 or 3 spatial dimensions, inferred; ``dims=2 | 3``: exactly that many.  The three flags are
    soft clDice's reading: only fp32 / fp16 / bf16 predictions, a multiclass target of the shape ``(B, *spatial)`` and not merely of its
    element count, no gradient into a dense target."""
    check_mode(what, mode)
    if not isinstance(y_pred, torch.Tensor) or not isinstance(y_true, torch.Tensor):
        raise TypeError(f"{what}: y_pred and y_true must be tensors")
    if half_or_single:
        if y_pred.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise TypeError(f"{what}: y_pred must be float32, float16 or bfloat16, got {y_pred.dtype}")
    elif not y_pred.is_floating_point():
        raise TypeError(f"{what}: y_pred must be a floating-point tensor, got {y_pred.dtype}")
    if dims is None:
        if y_pred.dim() - 2 not in (2, 3):
            raise ValueError(f"{what}: y_pred must be [B, C, H, W] or [B, C, D, H, W], got {tuple(y_pred.shape)}")
        layout = "*spatial"
    else:
        layout = "D, H, W" if dims == 3 else "H, W"
        if dims == 2 and y_pred.dim() == 5:
            raise NotImplementedError(f"{what}: 3-D volumes take dims=3 (the default dims=2 reads [B, C, H, W]); got {tuple(y_pred.shape)}")
        if y_pred.dim() != dims + 2:
            raise ValueError(f"{what}: y_pred must be [B, C, {layout}] for dims={dims}, got {tuple(y_pred.shape)}")
    B, C = y_pred.shape[0], y_pred.shape[1]
    spatial = tuple(y_pred.shape[2:])
    S = 1
    for n in spatial:
        S *= n
    if B * C * S == 0:
        raise ValueError(f"{what}: empty prediction of shape {tuple(y_pred.shape)}")
    if mode == BINARY_MODE and C != 1:
        raise ValueError(f"{what}: mode='binary' takes one channel, got {C}")
    if y_true.device != y_pred.device:
        y_true = y_true.to(y_pred.device)
    x = y_pred.float().contiguous().reshape(B, C, S)           # (fp16 / bf16 logits are widened first, like the other losses)
    labels = dense = None
    if mode == MULTICLASS_MODE:
        fits = tuple(y_true.shape) == (B,) + spatial if exact_labels else y_true.numel() == B * S
        if y_true.is_floating_point() or not fits:
            raise ValueError(f"{what}: a multiclass target holds integer labels [B, {layout}]; got {y_true.dtype} {tuple(y_true.shape)} for {tuple(y_pred.shape)}")
        labels = y_true.reshape(B, S).to(torch.int64).contiguous()
        prob = K.PROB_SOFTMAX if from_logits else K.PROB_IDENTITY
    else:
        if y_true.numel() != B * C * S:
            raise ValueError(f"{what}: target shape {tuple(y_true.shape)} does not match prediction shape {tuple(y_pred.shape)}")
        dense = (y_true.detach() if detach_target else y_true).float().contiguous().reshape(B, C, S)
        prob = K.PROB_SIGMOID if from_logits else K.PROB_IDENTITY
    has_ignore = ignore_index is not None
    ignore = (has_ignore, int(ignore_index) if has_ignore and labels is not None else 0, float(ignore_index) if has_ignore and dense is not None else 0.0)
    return Problem(x, labels, dense, prob, B, C, spatial, S, ignore)
