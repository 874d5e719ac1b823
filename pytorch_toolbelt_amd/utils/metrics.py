"""Confusion matrices of label maps and of logits, on the device the tensors are on, and the scores people quote from them.

The reference has no counterpart (it dropped its metrics module), so there is nothing to be a drop-in for: the names and meanings below
are this library's.  ``cm[t, p]`` counts the positions with ``target == t`` and ``pred == p``; per-class IoU / Dice, pixel accuracy and
mean IoU all derive from it (``segmentation_scores``).

CUDA tensors run the HIP kernels of ``csrc/ptb_confusion.hip`` (a missing kernel is an error, never a silent torch-op computation), CPU
tensors take torch ops with the same results -- the device the caller names decides.
"""
import torch

from .. import _native as N
from . import _maps as M

__all__ = ["confusion_matrix", "confusion_matrix_from_logits", "segmentation_scores"]

MAX_NATIVE_CLASSES = 256


# ---------------------------------------------------------------------------------------------------------------- validation
def _check_ignore(what, ignore_index):
    if ignore_index is None:
        return None
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, int):
        raise TypeError(f"{what}: ignore_index must be an int or None, got {ignore_index!r}")
    if not -(1 << 63) <= ignore_index < (1 << 63):
        raise ValueError(f"{what}: ignore_index {ignore_index} does not fit int64")
    return ignore_index


def _check_out(what, out, shape, device):
    if out is None:
        return
    if not isinstance(out, torch.Tensor):
        raise TypeError(f"{what}: out must be a tensor, got {type(out).__name__}")
    if out.dtype != torch.int64 or tuple(out.shape) != tuple(shape) or out.device != device:
        raise ValueError(f"{what}: out must be an int64 tensor of shape {tuple(shape)} on {device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    if not out.is_contiguous():
        raise ValueError(f"{what}: out must be contiguous (the counts are added to it in place)")


def _raise_invalid(what, count, K):
    if count:
        raise ValueError(f"{what}: {count} position(s) hold a target or pred outside [0, {K}) that is not ignore_index (strict=True)")


# ---------------------------------------------------------------------------------------------------------------- host form
def _count_host(pred2, target2, K, ignore_index):
    """[B, K, K] counts and the number of invalid positions of CPU ``[B, n]`` label tensors, by torch ops."""
    B = pred2.shape[0]
    p, t = pred2.to(torch.int64), target2.to(torch.int64)
    live = torch.ones_like(t, dtype=torch.bool) if ignore_index is None else t != ignore_index
    inside = (t >= 0) & (t < K) & (p >= 0) & (p < K)
    keep = live & inside
    idx = (torch.arange(B, dtype=torch.int64)[:, None] * K + t) * K + p
    cm = torch.bincount(idx[keep], minlength=B * K * K).view(B, K, K)
    return cm, int((live & ~inside).sum())


def _argmax_host(logits, threshold):
    """The prediction of CPU ``[N, C, *S]`` logits: first maximum wins, NaN counts as the maximum; ``C == 1``: ``logit > threshold``."""
    x = logits.to(torch.float32)
    if x.shape[1] == 1:
        return x[:, 0] > threshold
    nan = torch.isnan(x)
    clean = torch.where(nan, torch.full_like(x, float("inf")), x)           # every NaN is a maximum ...
    top = clean.max(dim=1, keepdim=True).values
    is_max = torch.where(nan.any(dim=1, keepdim=True), nan, clean == top)    # ... and with one present, only NaNs are
    return (is_max.cumsum(1) == 0).sum(1)                                    # the first of them


# ---------------------------------------------------------------------------------------------------------------- public
def confusion_matrix(pred, target, num_classes, ignore_index=None, per_sample=False, out=None, strict=False):
    """``int64 [K, K]`` with ``cm[t, p]`` = number of positions where ``target == t`` and ``pred == p`` (``K = num_classes``).

    ``pred`` / ``target``: integer label tensors (``bool``, ``uint8``, ``int16``, ``int32``, ``int64``; the two may differ) of equal shape,
    any rank, on one device.  ``per_sample=True``: the first dimension indexes samples and the result is ``[B, K, K]``.
    Values compare after widening to int64.  A position whose target equals ``ignore_index`` (any int64: 255, -100, a value inside
    ``[0, K)``) is skipped.  Any other position whose target or pred lies outside ``[0, K)`` is skipped too and counted on the device;
    ``strict=True`` reads that count back (8 bytes, the call's only D2H read) and raises ``ValueError`` with it.  With ``strict=False``
    nothing is read back: the call is stream-ordered and never synchronises.
    ``out``: an int64 tensor of the result's shape on the same device; the counts are ADDED to it and it is returned -- a validation
    epoch accumulates over batches without a host round trip.

    Contiguous CUDA inputs are read where they lie (no int64, boolean or combined-index copy); non-contiguous inputs are copied first.
    ``K <= 256`` is served natively; a larger ``K`` on a CUDA tensor raises ``NotImplementedError``.  Empty inputs give zeros (or ``out``
    unchanged) without a launch."""
    what = "confusion_matrix"
    M.check_labels(what, "pred", pred)
    M.check_labels(what, "target", target)
    if pred.shape != target.shape:
        raise ValueError(f"{what}: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    if pred.device != target.device:
        raise ValueError(f"{what}: pred is on {pred.device}, target on {target.device}")
    if isinstance(num_classes, bool) or not isinstance(num_classes, int):
        raise TypeError(f"{what}: num_classes must be an int, got {num_classes!r}")
    K = num_classes
    if K < 1:
        raise ValueError(f"{what}: num_classes must be >= 1, got {K}")
    ignore_index = _check_ignore(what, ignore_index)
    if per_sample and pred.dim() < 2:
        raise ValueError(f"{what}: per_sample needs a leading sample dimension, got shape {tuple(pred.shape)}")
    B = pred.shape[0] if per_sample else 1
    shape = (B, K, K) if per_sample else (K, K)
    _check_out(what, out, shape, pred.device)
    if pred.is_cuda and K > MAX_NATIVE_CLASSES:
        raise NotImplementedError(f"{what}: num_classes {K} > {MAX_NATIVE_CLASSES} has no native path; on the device use "
                                  "torch.bincount(target.long() * K + pred.long(), minlength=K * K).view(K, K)")
    if out is None:
        out = torch.zeros(shape, dtype=torch.int64, device=pred.device)
    n = pred.numel() // B if B else 0
    if B == 0 or n == 0:
        return out
    if pred.is_cuda:
        invalid = _labels_native(pred.contiguous(), target.contiguous(), B, n, K, ignore_index, out)
        if strict:
            _raise_invalid(what, int(invalid.item()), K)
    else:
        cm, invalid = _count_host(pred.reshape(B, n), target.reshape(B, n), K, ignore_index)
        if strict:
            _raise_invalid(what, invalid, K)
        out += cm.view(shape)
    return out


def _labels_native(pred, target, B, n, K, ignore_index, out):
    dev = pred.device
    invalid = torch.zeros(1, dtype=torch.int64, device=dev)
    N.launch("ptb_confusion_labels", dev, pred.data_ptr(), M.ELEM_BYTES[pred.dtype], target.data_ptr(), M.ELEM_BYTES[target.dtype], B, n, K,
             int(ignore_index is not None), ignore_index or 0, out.data_ptr(), invalid.data_ptr(), what="confusion_matrix")
    return invalid


def confusion_matrix_from_logits(logits, target, ignore_index=None, threshold=0.0, per_sample=False, out=None, strict=False):
    """The confusion matrix of a model output against ``target`` without materialising the prediction.

    ``logits``: ``[N, C, *S]`` in fp32, fp16 or bf16; ``target``: integer ``[N, *S]``.  ``C >= 2``: ``K = C`` (``<= 256`` on a CUDA tensor)
    and the prediction is the argmax over channels -- the first maximum wins and NaN counts as the maximum, the rule of
    ``merge_crop(argmax=True)`` -- so the result is ``confusion_matrix(argmax(logits, 1), target, C, ...)``.  ``C == 1``: ``K = 2`` and
    the prediction is ``logit > threshold`` (NaN gives 0).  ``ignore_index``, ``per_sample`` (``[N, K, K]``), ``out`` and ``strict`` as in
    ``confusion_matrix``.

    On a CUDA tensor the kernel reads the logits in the dtype the model wrote and widens in registers: no fp32 copy and no label map are
    written.  It reads dense ``[N, C, *S]`` memory; ``torch.channels_last`` / ``channels_last_3d`` (and any other strided) logits are
    copied to dense first."""
    what = "confusion_matrix_from_logits"
    if not isinstance(logits, torch.Tensor):
        raise TypeError(f"{what}: logits must be a tensor, got {type(logits).__name__}")
    if logits.dtype not in N.DTYPE_CODES:
        raise TypeError(f"{what}: logits must be float32, float16 or bfloat16, got {logits.dtype}")
    M.check_labels(what, "target", target)
    if logits.dim() < 2:
        raise ValueError(f"{what}: logits must be [N, C, *S], got {tuple(logits.shape)}")
    if tuple(target.shape) != (logits.shape[0],) + tuple(logits.shape[2:]):
        raise ValueError(f"{what}: target {tuple(target.shape)} does not match logits {tuple(logits.shape)} ([N, *S] against [N, C, *S])")
    if logits.device != target.device:
        raise ValueError(f"{what}: logits are on {logits.device}, target on {target.device}")
    Nb, C = logits.shape[0], logits.shape[1]
    if C < 1:
        raise ValueError(f"{what}: logits have no channel")
    ignore_index = _check_ignore(what, ignore_index)
    threshold = float(threshold)
    K = 2 if C == 1 else C
    shape = (Nb, K, K) if per_sample else (K, K)
    _check_out(what, out, shape, logits.device)
    if logits.is_cuda and C > MAX_NATIVE_CLASSES:
        raise NotImplementedError(f"{what}: {C} channels > {MAX_NATIVE_CLASSES} have no native path; on the device use "
                                  "torch.bincount(target.long() * C + logits.argmax(1).long(), minlength=C * C).view(C, C)")
    if out is None:
        out = torch.zeros(shape, dtype=torch.int64, device=logits.device)
    S = target.numel() // Nb if Nb else 0
    if Nb == 0 or S == 0:
        return out
    if logits.is_cuda:
        dev = logits.device
        dense, tgt = logits.contiguous(), target.contiguous()
        invalid = torch.zeros(1, dtype=torch.int64, device=dev)
        N.launch("ptb_confusion_logits", dev, dense.data_ptr(), N.DTYPE_CODES[dense.dtype], Nb, C, S, threshold, tgt.data_ptr(), M.ELEM_BYTES[tgt.dtype],
                 int(bool(per_sample)), int(ignore_index is not None), ignore_index or 0, out.data_ptr(), invalid.data_ptr(), what=what)
        if strict:
            _raise_invalid(what, int(invalid.item()), K)
    else:
        pred = _argmax_host(logits, threshold)
        B = Nb if per_sample else 1
        cm, invalid = _count_host(pred.reshape(B, -1), target.reshape(B, -1), K, ignore_index)
        if strict:
            _raise_invalid(what, invalid, K)
        out += cm.view(shape)
    return out


def segmentation_scores(cm):
    """The scores of a confusion matrix ``[..., K, K]`` (rows: target, columns: pred), as float64 torch ops on the matrix's device.

    Per class, ``[..., K]``, NaN where the denominator is 0: ``"iou"`` = tp / (tp + fp + fn), ``"dice"`` = 2 tp / (2 tp + fp + fn),
    ``"precision"`` = tp / (tp + fp), ``"recall"`` = tp / (tp + fn).  Of the whole matrix, ``[...]``: ``"accuracy"`` = trace / sum,
    ``"mean_iou"`` and ``"mean_dice"`` = the mean over the classes that are not NaN (NaN when there is none)."""
    if not isinstance(cm, torch.Tensor):
        raise TypeError(f"segmentation_scores: cm must be a tensor, got {type(cm).__name__}")
    if cm.dim() < 2 or cm.shape[-1] != cm.shape[-2]:
        raise ValueError(f"segmentation_scores: cm must be [..., K, K], got {tuple(cm.shape)}")
    m = cm.to(torch.float64)
    tp = m.diagonal(dim1=-2, dim2=-1)
    n_target, n_pred = m.sum(-1), m.sum(-2)
    fp, fn = n_pred - tp, n_target - tp
    iou = tp / (tp + fp + fn)
    dice = (2 * tp) / (2 * tp + fp + fn)
    return {"iou": iou, "dice": dice, "precision": tp / (tp + fp), "recall": tp / (tp + fn), "accuracy": tp.sum(-1) / m.sum((-2, -1)),
            "mean_iou": _nanmean(iou), "mean_dice": _nanmean(dice)}


def _nanmean(x):
    ok = ~torch.isnan(x)
    return torch.where(ok, x, torch.zeros_like(x)).sum(-1) / ok.sum(-1)
