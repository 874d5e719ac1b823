"""Hard-example mining: cross-entropy averaged over the hardest elements only -- top-k % (nnU-Net's ``TopKLoss``) and a threshold with a
floor on the kept count (OHEM: mmsegmentation's ``OHEMPixelSampler``, HRNet / OCR's ``OhemCrossEntropy``, BiSeNet's ``OhemCELoss``).  The
reference has no counterpart, so the names and meanings below are this library's.

THE ELEMENT LOSS is fp32 and never below +0:

    multiclass            l = (max_c x_c - x_label) + log(sum_c exp(x_c - max_c))           one element per position
    binary / multilabel   l = max(x, 0) - x g + log1p(exp(-|x|))                             one element per (channel, position)

Elements whose label (target) equals ``ignore_index`` are in no selection set, no sum and no count.  A SELECTION SET is every other
element of the batch (``per_sample=False``, a 0-dim result) or of one sample (``per_sample=True``: ``reduction="mean"`` averages the B
values, ``"none"`` returns ``[B]``); ``n`` is its size.

    top-k   kept = max(1, floor(float64(n) * k / 100)), 0 < k <= 100
    OHEM    t0 = float32(-log(thresh)); with m = min(min_kept, n): the elements with l > t0 if there are at least m of them (kept is
            their number), the m largest otherwise.  This is mmsegmentation's rule stated on the loss instead of on the probability
            of the label; at an exact tie with the threshold the kept count can differ by one from published code.

The loss is the mean of the ``kept`` largest element losses; a set with nothing kept (``n == 0``, or ``min_kept == 0`` with nothing above
``t0``) gives 0 and a zero gradient.  TIES AT THE CUT: with ``thr`` the smallest kept value, ``gt`` the number of losses above it and
``eq`` the number equal to it by bits, the loss is ``(sum_{l > thr} l + (kept - gt) thr) / kept`` -- what any tie-break gives -- and in
the gradient the ``eq`` tied elements share the ``kept - gt`` places equally, weight ``(kept - gt) / eq`` each: a valid subgradient,
independent of launch order.  ``torch.topk`` picks an unspecified subset among ties, so this is the one place where the gradient (not
the value) differs from the chain ``F.cross_entropy(reduction="none") -> flatten -> topk -> mean``.

CUDA tensors run the HIP kernels of ``csrc/ptb_hard_mining.hip`` (a missing kernel is an error, never a silent host computation): one
streaming pass writes the element-loss map and the first histogram, a four-pass radix select finds ``thr`` without a sort and without
a read-back, and the backward is one more pass that reads the saved map for the decision.  CPU tensors take the torch ops below: the
same definitions.

Left out: class weights, label smoothing and soft multiclass targets, a selection across the ranks of ``parallel.py``'s batch-sharded
losses, native fp16 / bf16 reads (such logits are widened first, like in the other losses)."""
import math
from typing import Optional

import numpy as np
import torch
from torch import Tensor
from torch.nn.modules.loss import _Loss

from .. import _native as N
from . import _kernels as K
from ._region import BINARY_MODE, MULTICLASS_MODE, MULTILABEL_MODE
from .distance_losses import _problem

__all__ = ["TopKCrossEntropyLoss", "OhemCrossEntropyLoss", "topk_cross_entropy", "ohem_cross_entropy"]

TOPK, OHEM = 0, 1                    # PTB_HARDCE_*
_NAMES = {TOPK: "topk_cross_entropy", OHEM: "ohem_cross_entropy"}


# ---------------------------------------------------------------------------------------------------------------- arguments
def _rule(what, rule, k, thresh, min_kept, per_sample, reduction):
    """``(rule, k, t0, min_kept)`` as the kernels take them"""
    if reduction not in ("mean", "none"):
        raise ValueError(f"{what}: reduction must be 'mean' or 'none', got {reduction!r}")
    if reduction == "none" and not per_sample:
        raise ValueError(f"{what}: reduction='none' returns one value per sample and requires per_sample=True")
    if rule == TOPK:
        k = float(k)
        if not 0.0 < k <= 100.0:
            raise ValueError(f"{what}: k is a percentage in (0, 100], got {k}")
        return rule, k, 0.0, 0
    thresh = float(thresh)
    if not 0.0 < thresh < 1.0:
        raise ValueError(f"{what}: thresh is a probability in (0, 1), got {thresh}")
    if int(min_kept) != min_kept or min_kept < 0:
        raise ValueError(f"{what}: min_kept must be an integer >= 0, got {min_kept}")
    t0 = float(np.float32(-math.log(thresh)))              # float64 on the host, rounded once (> 0 for every float64 below 1)
    return rule, 0.0, t0, int(min_kept)


# ---------------------------------------------------------------------------------------------------------------- device
class HardMinedCrossEntropy(torch.autograd.Function):
    """The whole loss as one node: ``ptb_hardce_fwd``; backward ``ptb_hardce_bwd``.  Saves the logits, the target, the element-loss map (4
    bytes per element) and the small state of every set.  Stream-ordered, no read-back.  Returns ``(loss, thr, kept)`` of every set."""

    @staticmethod
    def forward(ctx, x, labels, dense, cfg):
        what, rule, k, t0, min_kept, ignore, per_sample = cfg
        B, C, S = x.shape
        has_ignore, ignore_label, ignore_value = ignore
        nbytes = N.load().ptb_hardce_workspace_bytes(int(dense is not None), B, C, S, int(per_sample))
        if nbytes < 0:
            N.check(int(nbytes), what)
        sets = B if per_sample else 1
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        emap = torch.empty((B, S) if labels is not None else (B, C, S), dtype=torch.float32, device=x.device)
        loss = torch.empty(sets, dtype=torch.float32, device=x.device)
        thr = torch.empty(sets, dtype=torch.float32, device=x.device)
        kept = torch.empty(sets, dtype=torch.int64, device=x.device)
        inv = torch.empty(sets, dtype=torch.float32, device=x.device)
        select = torch.empty((sets, 2), dtype=torch.int32, device=x.device)
        flag = torch.empty(1, dtype=torch.int32, device=x.device)
        N.launch("ptb_hardce_fwd", x.device, x.data_ptr(), N.ptr(labels), N.ptr(dense), B, C, S, int(has_ignore), ignore_label, ignore_value,
                 int(per_sample), rule, k, t0, min_kept, emap.data_ptr(), ws.data_ptr(), ws.numel(), loss.data_ptr(), thr.data_ptr(),
                 kept.data_ptr(), inv.data_ptr(), select.data_ptr(), flag.data_ptr(), what=what)
        if labels is not None:
            K.check_labels(flag)
        ctx.save_for_backward(x, labels, dense, emap, inv, select)
        ctx.cfg = (what, per_sample)
        if not per_sample:
            loss, thr, kept = loss.reshape(()), thr.reshape(()), kept.reshape(())
        ctx.mark_non_differentiable(thr, kept)
        return loss, thr, kept

    @staticmethod
    def backward(ctx, g, _thr, _kept):
        x, labels, dense, emap, inv, select = ctx.saved_tensors
        what, per_sample = ctx.cfg
        B, C, S = x.shape
        coef = (g.reshape(-1).to(torch.float32) * inv).contiguous()        # upstream gradient / kept, on the device
        grad = torch.empty_like(x)
        N.launch("ptb_hardce_bwd", x.device, x.data_ptr(), N.ptr(labels), N.ptr(dense), emap.data_ptr(), B, C, S, int(per_sample), coef.data_ptr(),
                 select.data_ptr(), grad.data_ptr(), what=what)
        return grad, None, None, None


# ---------------------------------------------------------------------------------------------------------------- host
def _host_kept(rule, n, above, k, min_kept):
    if n == 0:
        return 0
    if rule == TOPK:
        return min(n, max(1, int(math.floor(float(n) * k / 100.0))))
    floor = min(min_kept, n)
    return above if above >= floor else floor


def _host_loss(x, labels, dense, rule, k, t0, min_kept, ignore, per_sample):
    """The definitions in torch ops: ``thr`` from ``kthvalue`` on the detached element losses, the weights 1 / tie weight / 0 detached, so
    that autograd yields the tie gradient of the device form.  The element losses are evaluated in float64 and rounded to float32 ONCE
    for the selection: torch's vectorised float32 kernels give bit-identical logit vectors different bits in their vector and
    remainder loops, which would split a tie."""
    B, C, S = x.shape
    has_ignore, ignore_label, ignore_value = ignore
    xd = x.double()
    if labels is not None:
        valid = labels != ignore_label if has_ignore else torch.ones_like(labels, dtype=torch.bool)
        if bool(((labels < 0) | (labels >= C))[valid].any()):
            raise RuntimeError(K.LABEL_MSG)
        m = xd.max(dim=1).values
        xl = xd.gather(1, torch.where(valid, labels, torch.zeros_like(labels)).unsqueeze(1)).squeeze(1)
        l = (m - xl) + torch.log(torch.exp(xd - m.unsqueeze(1)).sum(dim=1))
    else:
        valid = dense != ignore_value if has_ignore else torch.ones_like(dense, dtype=torch.bool)
        g = torch.where(valid, dense, torch.zeros_like(dense)).double()
        l = (xd.clamp_min(0) - xd * g) + torch.log1p(torch.exp(-xd.abs()))
    l = l.reshape(B, -1)
    valid = valid.reshape(B, -1)
    if not per_sample:
        l, valid = l.reshape(1, -1), valid.reshape(1, -1)
    losses, thrs, kepts = [], [], []
    for ls, vs in zip(l, valid):
        v = ls[vs]
        d = v.detach().float().clamp_min(0.0)              # the fp32 element losses the selection orders (+0 for -0)
        n = int(d.numel())
        kept = _host_kept(rule, n, int((d > t0).sum()) if rule == OHEM else 0, k, min_kept)
        kepts.append(kept)
        if kept == 0:
            losses.append((ls.sum() * 0.0).float())
            thrs.append(torch.tensor(float("inf"), dtype=torch.float32))
            continue
        thr = d.kthvalue(n - kept + 1).values
        gt, eq = int((d > thr).sum()), int((d == thr).sum())
        w = (d > thr).to(torch.float64) + (d == thr).to(torch.float64) * ((kept - gt) / eq)
        losses.append(((v * w).sum() / kept).float())
        thrs.append(thr)
    loss, thr, kept = torch.stack(losses), torch.stack(thrs), torch.tensor(kepts, dtype=torch.int64)
    if not per_sample:
        loss, thr, kept = loss.reshape(()), thr.reshape(()), kept.reshape(())
    return loss, thr, kept


# ---------------------------------------------------------------------------------------------------------------- public
def _loss(rule, y_pred, y_true, mode, k, thresh, min_kept, ignore_index, per_sample, reduction, return_threshold):
    what = _NAMES[rule]
    rule, k, t0, min_kept = _rule(what, rule, k, thresh, min_kept, per_sample, reduction)
    x, labels, dense, _, _, _, _, ignore, _ = _problem(what, y_pred, y_true, mode, None, True, ignore_index, None, None)
    per_sample = bool(per_sample)
    if x.is_cuda:
        loss, thr, kept = HardMinedCrossEntropy.apply(x, labels, dense, (what, rule, k, t0, min_kept, ignore, per_sample))
    else:
        loss, thr, kept = _host_loss(x, labels, dense, rule, k, t0, min_kept, ignore, per_sample)
    if per_sample and reduction == "mean":
        loss = loss.mean()
    return (loss, thr, kept) if return_threshold else loss


def topk_cross_entropy(y_pred, y_true, mode=MULTICLASS_MODE, k=10.0, ignore_index=None, per_sample=False, reduction="mean", return_threshold=False):
    """The mean of the ``k`` % largest element cross-entropies: see ``TopKCrossEntropyLoss``.  ``return_threshold=True`` also returns the
    smallest kept loss (float32, 0-dim or ``[B]``, +inf for an empty kept set) and the kept count (int64), both on the device of the input."""
    return _loss(TOPK, y_pred, y_true, mode, k, None, None, ignore_index, per_sample, reduction, return_threshold)


def ohem_cross_entropy(y_pred, y_true, mode=MULTICLASS_MODE, thresh=0.7, min_kept=100_000, ignore_index=None, per_sample=False, reduction="mean",
                       return_threshold=False):
    """The mean of the element cross-entropies above ``-log(thresh)``, of the ``min_kept`` largest when fewer are: see
    ``OhemCrossEntropyLoss``.  ``return_threshold`` as in ``topk_cross_entropy``."""
    return _loss(OHEM, y_pred, y_true, mode, None, thresh, min_kept, ignore_index, per_sample, reduction, return_threshold)


class _HardMinedLoss(_Loss):
    _rule = TOPK

    def __init__(self, mode, k, thresh, min_kept, ignore_index, per_sample, reduction):
        what = type(self).__name__
        if mode not in (BINARY_MODE, MULTICLASS_MODE, MULTILABEL_MODE):
            raise ValueError(f"{what}: mode must be 'binary', 'multiclass' or 'multilabel', got {mode!r}")
        _rule(what, self._rule, k, thresh, min_kept, per_sample, reduction)
        super().__init__()
        self.mode = mode
        self.k = None if k is None else float(k)
        self.thresh = None if thresh is None else float(thresh)
        self.min_kept = None if min_kept is None else int(min_kept)
        self.ignore_index = ignore_index
        self.per_sample = bool(per_sample)
        self.reduction = reduction

    def forward(self, y_pred: Tensor, y_true: Tensor) -> Tensor:
        return _loss(self._rule, y_pred, y_true, self.mode, self.k, self.thresh, self.min_kept, self.ignore_index, self.per_sample, self.reduction, False)


class TopKCrossEntropyLoss(_HardMinedLoss):
    """Cross-entropy averaged over the ``k`` % hardest elements: ``kept = max(1, floor(n k / 100))`` of the ``n`` elements that are not
    ignored, the mean of the ``kept`` largest element losses.

    ``mode``: ``"multiclass"`` (logits ``[B, C, *spatial]``, integer labels ``[B, *spatial]``, softmax cross-entropy, an element per
    position), ``"binary"`` (``[B, 1, *spatial]``) or ``"multilabel"`` (dense float targets in [0, 1] of the logits' shape, sigmoid
    cross-entropy, an element per channel and position); 2 or 3 spatial dimensions, inferred.  ``per_sample``: select inside every sample
    instead of over the batch; ``reduction``: ``"mean"``, or ``"none"`` (``[B]``; requires ``per_sample=True``).  Ties at the cut share
    the remaining places equally (see the module docstring)."""

    _rule = TOPK

    def __init__(self, mode: str = MULTICLASS_MODE, k: float = 10.0, ignore_index: Optional[int] = None, per_sample: bool = False,
                 reduction: str = "mean"):
        super().__init__(mode, k, None, None, ignore_index, per_sample, reduction)


class OhemCrossEntropyLoss(_HardMinedLoss):
    """Online hard example mining: the mean of the element cross-entropies above ``t0 = -log(thresh)`` -- the elements whose label has a
    probability below ``thresh`` -- and, when fewer than ``min(min_kept, n)`` are, of the ``min(min_kept, n)`` largest.  ``min_kept``
    counts elements of a selection set: of the batch, or with ``per_sample=True`` of every sample.  Other arguments as
    ``TopKCrossEntropyLoss``."""

    _rule = OHEM

    def __init__(self, mode: str = MULTICLASS_MODE, thresh: float = 0.7, min_kept: int = 100_000, ignore_index: Optional[int] = None,
                 per_sample: bool = False, reduction: str = "mean"):
        super().__init__(mode, None, thresh, min_kept, ignore_index, per_sample, reduction)
