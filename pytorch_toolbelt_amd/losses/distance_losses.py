"""Distance-map losses on the device-side distance transform: the boundary loss (Kervadec et al., MIDL 2019) and the Hausdorff-DT loss
(Karimi & Salcudean, TMI 2019).  The reference has no counterpart, so the names and meanings below are this library's.

With ``p`` the activation of the logits, ``g`` the 0 / 1 target and ``phi_k`` the SIGNED distance map of class ``k`` of a sample --
``utils.distance_transform(..., foreground=k, signed=True)``: positive outside the object, negative inside, the boundary positions inside
at -1 (Kervadec's reference code uses ``d - 1`` inside, which puts them at 0) --

    boundary      term = p_k * phi_truth,k
    Hausdorff-DT  term = (p_k - g_k)^2 * (|phi_pred,k|^alpha + |phi_truth,k|^alpha),   phi_pred of the object ``p_k > 0.5``

and the loss is the mean of the terms over (batch, selected classes, positions that are not ignored); ``reduction="none"`` gives that
mean per sample, ``[B]``.  A map WITHOUT A BOUNDARY -- a sample that lacks the class, or is the class everywhere; the transform leaves
+-inf there -- counts as 0: such a sample contributes nothing for that class instead of ``inf`` (the ``if mask.any()`` of the published
implementations).  Positions that hold ``ignore_index`` belong to no object for the transform and are left out of sum and count.  No
gradient flows through a distance transform: the maps are constants.

CUDA tensors run the HIP kernels of ``csrc/ptb_distance_loss.hip`` around ``ptb_edt`` (a missing kernel is an error, never a silent host
computation): one launch writes the object maps of all classes (and of the thresholded prediction), ONE transform runs over all of
them, one streaming pass evaluates the loss with the activation in registers, and the backward is one more pass.  CPU tensors take the
torch ops below on the numpy transform: the same definitions."""
from typing import List, Optional

import numpy as np
import torch
from torch import Tensor
from torch.nn.modules.loss import _Loss

from .. import _native as N
from ..utils import _maps as M
from ..utils import distance as _distance
from . import _kernels as K
from ._region import BINARY_MODE, MULTICLASS_MODE, MULTILABEL_MODE

__all__ = ["BoundaryLoss", "HausdorffDTLoss", "boundary_loss", "hausdorff_dt_loss"]

BOUNDARY, HAUSDORFF = 0, 1           # PTB_DLOSS_*
_MAPS_I32_SQUARED, _MAPS_F32 = 0, 1
_NAMES = {BOUNDARY: "boundary_loss", HAUSDORFF: "hausdorff_dt_loss"}


# ---------------------------------------------------------------------------------------------------------------- arguments
def _problem(what, y_pred, y_true, mode, classes, from_logits, ignore_index, spacing, dist_maps):
    """The tensors as the kernels take them -- x fp32 ``[B, C, S]``, labels int64 ``[B, S]`` or dense fp32 ``[B, C, S]`` -- and the rest of a call."""
    if mode not in (BINARY_MODE, MULTICLASS_MODE, MULTILABEL_MODE):
        raise ValueError(f"{what}: mode must be 'binary', 'multiclass' or 'multilabel', got {mode!r}")
    if not isinstance(y_pred, torch.Tensor) or not isinstance(y_true, torch.Tensor):
        raise TypeError(f"{what}: y_pred and y_true must be tensors")
    if not y_pred.is_floating_point():
        raise TypeError(f"{what}: y_pred must be a floating-point tensor, got {y_pred.dtype}")
    dims = y_pred.dim() - 2
    if dims not in (2, 3):
        raise ValueError(f"{what}: y_pred must be [B, C, H, W] or [B, C, D, H, W], got {tuple(y_pred.shape)}")
    B, C = y_pred.shape[0], y_pred.shape[1]
    spatial = tuple(y_pred.shape[2:])
    S = int(np.prod(spatial))
    if B * C * S == 0:
        raise ValueError(f"{what}: empty prediction of shape {tuple(y_pred.shape)}")
    if mode == BINARY_MODE and C != 1:
        raise ValueError(f"{what}: mode='binary' takes one channel, got {C}")
    if y_true.device != y_pred.device:
        y_true = y_true.to(y_pred.device)
    x = y_pred.float().contiguous().reshape(B, C, S)          # (fp16 / bf16 logits are widened first, like the other losses)
    labels = dense = None
    if mode == MULTICLASS_MODE:
        if y_true.is_floating_point() or y_true.numel() != B * S:
            raise ValueError(f"{what}: a multiclass target holds integer labels [B, *spatial]; got {y_true.dtype} {tuple(y_true.shape)} for {tuple(y_pred.shape)}")
        labels = y_true.reshape(B, S).to(torch.int64).contiguous()
        prob = K.PROB_SOFTMAX if from_logits else K.PROB_IDENTITY
    else:
        if y_true.numel() != B * C * S:
            raise ValueError(f"{what}: target shape {tuple(y_true.shape)} does not match prediction shape {tuple(y_pred.shape)}")
        dense = y_true.float().contiguous().reshape(B, C, S)
        prob = K.PROB_SIGMOID if from_logits else K.PROB_IDENTITY
    table = _distance.class_table(what, classes, C, x.device)
    sp = M.spacing(what, spacing, dims)
    D = spatial[0] if dims == 3 else 1
    geometry = (dims, D, spatial[-2], spatial[-1])
    if dist_maps is not None:
        want = (B, table[0]) + spatial
        if not isinstance(dist_maps, torch.Tensor) or tuple(dist_maps.shape) != want or dist_maps.device != x.device:
            raise ValueError(f"{what}: dist_maps must be the [B, K, *spatial] = {want} output of class_distance_maps on {x.device}")
        if dist_maps.dtype == torch.int32 and sp is None:
            pass                                               # the exact squared integers of squared=True
        elif dist_maps.dtype != torch.float32:
            raise TypeError(f"{what}: dist_maps must be float32 distances, or with unit spacing the int32 of squared=True; got {dist_maps.dtype}")
        dist_maps = dist_maps.contiguous().reshape(B, table[0], S)
    has_ignore = ignore_index is not None
    ignore = (has_ignore, int(ignore_index) if has_ignore and labels is not None else 0, float(ignore_index) if has_ignore and dense is not None else 0.0)
    return x, labels, dense, prob, table, sp, geometry, ignore, dist_maps


# ---------------------------------------------------------------------------------------------------------------- device
class DistanceMapLoss(torch.autograd.Function):
    """The whole loss as one node: ``ptb_dloss_masks``, one ``ptb_edt`` per chunk, ``ptb_dloss_fwd``; backward ``ptb_dloss_bwd``.  Saves the
    logits, the target and the map(s) (4 bytes per position and selected class, twice that for Hausdorff).  Stream-ordered, no read-back."""

    @staticmethod
    def forward(ctx, x, labels, dense, dist_maps, cfg):
        kind, prob, table, sp, geometry, ignore, alpha, per_sample, cap = cfg
        what = _NAMES[kind]
        B, C, S = x.shape
        Kn, _, host, dev_table = table
        has_ignore, ignore_label, ignore_value = ignore
        dims, D, H, W = geometry
        planes = (0 if dist_maps is not None else _distance.PLANE_TRUTH) | (_distance.PLANE_PRED if kind == HAUSDORFF else 0)
        truth, pred = dist_maps, None
        if planes:
            maps, _ = _distance.signed_maps_device(what, x, labels, dense, C, table, planes, prob, has_ignore, ignore_label, ignore_value, dims, D, H, W,
                                                   sp, sp is None and (dist_maps is None or dist_maps.dtype == torch.int32), cap)
            if dist_maps is None:
                truth = maps[0]
            if kind == HAUSDORFF:
                pred = maps[-1]                    # (in the form of the caller's maps: float32 distances, or the squared integers)
        maps_kind = _MAPS_I32_SQUARED if truth.dtype == torch.int32 else _MAPS_F32
        _, _, slots = _distance.plan_maps(what, N.load(), dims, B, D, H, W, Kn, 1, 1 << 62)
        results = B if per_sample else 1
        ws = M.scratch(16 * slots, x.device)
        loss = torch.empty(results, dtype=torch.float32, device=x.device)
        inv = torch.empty(results, dtype=torch.float32, device=x.device)
        flag = torch.empty(1, dtype=torch.int32, device=x.device)
        N.launch("ptb_dloss_fwd", x.device, kind, x.data_ptr(), N.ptr(labels), N.ptr(dense), host, N.ptr(dev_table), truth.data_ptr(), N.ptr(pred),
                 maps_kind, B, C, Kn, S, prob, int(has_ignore), ignore_label, ignore_value, alpha, int(per_sample),
                 ws.data_ptr(), ws.numel(), loss.data_ptr(), inv.data_ptr(), flag.data_ptr(), what=what)
        if labels is not None:
            K.check_labels(flag)
        ctx.save_for_backward(x, labels, dense, truth, pred, inv, dev_table)
        ctx.cfg = (kind, prob, host, Kn, ignore, alpha, per_sample, maps_kind)
        return loss if per_sample else loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        x, labels, dense, truth, pred, inv, dev_table = ctx.saved_tensors
        kind, prob, host, Kn, ignore, alpha, per_sample, maps_kind = ctx.cfg
        has_ignore, ignore_label, ignore_value = ignore
        B, C, S = x.shape
        coef = (g.reshape(-1).to(torch.float32) * inv).contiguous()        # upstream gradient / count, on the device
        grad = torch.empty_like(x)
        N.launch("ptb_dloss_bwd", x.device, kind, x.data_ptr(), N.ptr(labels), N.ptr(dense), host, N.ptr(dev_table), truth.data_ptr(), N.ptr(pred),
                 maps_kind, B, C, Kn, S, prob, int(has_ignore), ignore_label, ignore_value, alpha, int(per_sample),
                 coef.data_ptr(), grad.data_ptr(), what=_NAMES[kind])
        return grad, None, None, None, None


# ---------------------------------------------------------------------------------------------------------------- host
def _finite(t):
    return torch.where(torch.isfinite(t), t, torch.zeros_like(t))


def _host_distances(maps, S):
    """float64 ``[B, K, S]`` |distance| and sign of maps in either form, an entry without a boundary as 0"""
    m = maps.reshape(maps.shape[0], maps.shape[1], S)
    if m.dtype == torch.int32:
        m = m.to(torch.float64)
        m = torch.where(m.abs() >= float(_distance.INT_INF), torch.zeros_like(m), m)
        return m.abs().sqrt(), m.sign()
    m = _finite(m.to(torch.float64))
    return m.abs(), m.sign()


def _host_loss(kind, x, labels, dense, prob, table, sp, geometry, ignore, dist_maps, alpha, per_sample):
    B, C, S = x.shape
    Kn, cls, _, _ = table
    cls = list(cls) if cls is not None else list(range(C))
    has_ignore, ignore_label, ignore_value = ignore
    dims, D, H, W = geometry
    p = torch.softmax(x, dim=1) if prob == K.PROB_SOFTMAX else torch.sigmoid(x) if prob == K.PROB_SIGMOID else x
    p = p[:, cls]
    if labels is not None:
        valid = (labels != ignore_label if has_ignore else torch.ones_like(labels, dtype=torch.bool)).unsqueeze(1).expand(B, Kn, S)
        g = labels.unsqueeze(1) == torch.tensor(cls, dtype=torch.int64).reshape(1, Kn, 1)
    else:
        d = dense[:, cls]
        valid = d != ignore_value if has_ignore else torch.ones_like(d, dtype=torch.bool)
        g = d > 0.5
    objects = g & valid

    def transform(obj):
        maps = _distance.signed_maps_host(obj.numpy().reshape(B * Kn, D, H, W), sp, sp is None)
        return torch.from_numpy(maps).reshape(B, Kn, S)

    dt, st = _host_distances(dist_maps if dist_maps is not None else transform(objects), S)
    if kind == BOUNDARY:
        term = p * (dt * st).to(p.dtype)
    else:
        dp, _ = _host_distances(transform(p.detach() > 0.5), S)
        term = (p - g.to(p.dtype)) ** 2 * (dp ** alpha + dt ** alpha).to(p.dtype)
    term = term * valid.to(term.dtype)
    if per_sample:
        return term.sum(dim=(1, 2)) / valid.sum(dim=(1, 2)).to(term.dtype)
    return term.sum() / valid.sum().to(term.dtype)


# ---------------------------------------------------------------------------------------------------------------- public
def _loss(kind, y_pred, y_true, mode, classes, from_logits, ignore_index, spacing, reduction, dist_maps, alpha, max_workspace_bytes):
    what = _NAMES[kind]
    if reduction not in ("mean", "none"):
        raise ValueError(f"{what}: reduction must be 'mean' or 'none', got {reduction!r}")
    alpha = float(alpha)
    if not (alpha > 0.0 and np.isfinite(alpha)):
        raise ValueError(f"{what}: alpha must be positive and finite, got {alpha}")
    x, labels, dense, prob, table, sp, geometry, ignore, dist_maps = _problem(what, y_pred, y_true, mode, classes, from_logits, ignore_index, spacing,
                                                                              dist_maps)
    per_sample = reduction == "none"
    if not x.is_cuda:
        return _host_loss(kind, x, labels, dense, prob, table, sp, geometry, ignore, dist_maps, alpha, per_sample)
    cfg = (kind, prob, table, sp, geometry, ignore, alpha, per_sample, int(max_workspace_bytes))
    return DistanceMapLoss.apply(x, labels, dense, dist_maps, cfg)


def boundary_loss(y_pred, y_true, mode=MULTICLASS_MODE, classes=None, from_logits=True, ignore_index=None, spacing=None, reduction="mean",
                  dist_maps=None, max_workspace_bytes=_distance.DEFAULT_WORKSPACE_CAP):
    """``mean(p_k * phi_k)`` over (batch, ``classes``, positions that are not ignored): see ``BoundaryLoss``."""
    return _loss(BOUNDARY, y_pred, y_true, mode, classes, from_logits, ignore_index, spacing, reduction, dist_maps, 2.0, max_workspace_bytes)


def hausdorff_dt_loss(y_pred, y_true, mode=MULTICLASS_MODE, classes=None, from_logits=True, ignore_index=None, spacing=None, reduction="mean",
                      alpha=2.0, dist_maps=None, max_workspace_bytes=_distance.DEFAULT_WORKSPACE_CAP):
    """``mean((p_k - g_k)^2 (|phi_pred,k|^alpha + |phi_truth,k|^alpha))``: see ``HausdorffDTLoss``."""
    return _loss(HAUSDORFF, y_pred, y_true, mode, classes, from_logits, ignore_index, spacing, reduction, dist_maps, alpha, max_workspace_bytes)


class _DistanceLoss(_Loss):
    _kind = BOUNDARY

    def __init__(self, mode: str, classes: Optional[List[int]] = None, from_logits: bool = True, ignore_index: Optional[int] = None, spacing=None,
                 reduction: str = "mean", alpha: float = 2.0):
        what = type(self).__name__
        if mode not in (BINARY_MODE, MULTICLASS_MODE, MULTILABEL_MODE):
            raise ValueError(f"{what}: mode must be 'binary', 'multiclass' or 'multilabel', got {mode!r}")
        if classes is not None and mode == BINARY_MODE:
            raise ValueError(f"{what}: masking classes is not supported with mode='binary'")
        if reduction not in ("mean", "none"):
            raise ValueError(f"{what}: reduction must be 'mean' or 'none', got {reduction!r}")
        if not (float(alpha) > 0.0 and np.isfinite(float(alpha))):
            raise ValueError(f"{what}: alpha must be positive and finite, got {alpha}")
        super().__init__()
        self.mode = mode
        self.classes = None if classes is None else [int(c) for c in classes]
        if self.classes is not None and (not self.classes or len(set(self.classes)) != len(self.classes) or min(self.classes) < 0):
            raise ValueError(f"{what}: classes must be distinct non-negative ints, got {classes!r}")
        self.from_logits = bool(from_logits)
        self.ignore_index = ignore_index
        self.spacing = None if spacing is None else tuple(float(v) for v in spacing)
        if self.spacing is not None and (len(self.spacing) not in (2, 3) or not all(np.isfinite(v) and v > 0 for v in self.spacing)):
            raise ValueError(f"{what}: spacing must be 2 or 3 positive finite floats, got {spacing!r}")
        self.reduction = reduction
        self.alpha = float(alpha)

    def forward(self, y_pred: Tensor, y_true: Tensor, dist_maps: Optional[Tensor] = None) -> Tensor:
        return _loss(self._kind, y_pred, y_true, self.mode, self.classes, self.from_logits, self.ignore_index, self.spacing, self.reduction, dist_maps,
                     self.alpha, _distance.DEFAULT_WORKSPACE_CAP)


class BoundaryLoss(_DistanceLoss):
    """Boundary loss: ``mean(p_k * phi_k)``, ``phi_k`` the signed distance map of class ``k`` of the target (> 0 outside, < 0 inside).

    ``mode``: ``"binary"`` (logits ``[B, 1, *spatial]``, target of the same size, object where > 0.5), ``"multiclass"`` (logits ``[B, C,
    *spatial]``, integer labels ``[B, *spatial]``, softmax) or ``"multilabel"`` (dense targets ``[B, C, *spatial]``, sigmoid); 2 or 3
    spatial dimensions, inferred.  ``classes``: the channels that count (Kervadec's usual setting leaves the background out:
    ``classes=[1, ..., C - 1]``).  ``from_logits=False``: ``y_pred`` already holds probabilities.  ``ignore_index``: positions that hold
    it belong to no object and are left out of the mean.  ``spacing``: as ``utils.distance_transform``.  ``reduction``: ``"mean"`` or
    ``"none"`` (``[B]``, the mean of every sample).

    ``forward(y_pred, y_true, dist_maps=None)``: ``dist_maps`` is the output of ``utils.class_distance_maps`` for the same classes, spacing
    and ignore_index -- ``squared=True`` with unit spacing (the exact integers: the same bits as without), the distances with
    ``spacing`` -- and saves the transform: the boundary loss then launches none."""

    _kind = BOUNDARY

    def __init__(self, mode: str, classes: Optional[List[int]] = None, from_logits: bool = True, ignore_index: Optional[int] = None, spacing=None,
                 reduction: str = "mean"):
        super().__init__(mode, classes, from_logits, ignore_index, spacing, reduction)


class HausdorffDTLoss(_DistanceLoss):
    """Hausdorff-DT loss: ``mean((p_k - g_k)^2 * (|phi_pred,k|^alpha + |phi_truth,k|^alpha))``; ``phi_pred`` is the signed distance map of
    the object ``p_k > 0.5`` (the threshold is fixed), transformed in every step together with the target's maps in one call.  Arguments as
    ``BoundaryLoss``, and ``alpha`` (2.0: the exact squared integers without a root).  With ``dist_maps=`` only the prediction is
    transformed."""

    _kind = HAUSDORFF
