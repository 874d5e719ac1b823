"""The soft-clDice training loss (Shit et al., "clDice -- a Novel Topology-Preserving Loss Function for Tubular Structure Segmentation",
CVPR 2021) for vessels, roads, neurites and cracks, with its gradient.  The reference has no counterpart, so the names and meanings
below are this library's; ``utils.centerline_dice`` is the hard metric of the same name.

DEFINITION (these formulae are the definition).  For one plane ``x`` of ``H x W`` values in ``[0, 1]`` and ``k = iterations``: ``E(x)(p)`` is the minimum of
``x`` over ``p`` and its 4 edge neighbours inside the plane, ``D(x)(p)`` the maximum over the 3 x 3 window inside the plane; positions outside the
plane never take part::

    v_0 = x    v_j+1 = E(v_j)    o_j = D(v_j+1)    delta_j = relu(v_j - o_j)     j = 0 .. k
    S_0 = delta_0    S_j = S_j-1 + relu(delta_j - S_j-1 delta_j)                 softskel_k(x) = S_k

-- the published ``soft_skel`` (jocpae/clDice): ``k + 1`` erosions and ``k + 1`` dilations.  With ``p`` the activation of the logits, ``g`` the 0 / 1 (or dense)
target of a selected class ``c``, ``SP = softskel_k(p_c)``, ``ST = softskel_k(g_c)`` and all sums over batch and positions of class ``c``::

    tprec_c = (sum SP g + smooth) / (sum SP + smooth)      tsens_c = (sum ST p + smooth) / (sum ST + smooth)
    loss_c  = 1 - 2 tprec_c tsens_c / (tprec_c + tsens_c)  loss    = mean of loss_c over the selected classes

Per class and then the mean, like ``DiceLoss`` here: for ``binary`` mode or one selected class this is the published value; the paper pools
all foreground channels into one set of sums instead (left out).

VOLUMES (``dims=3``).  For one volume ``x`` of ``D x H x W`` values the chain, the loss and the mean are the same and only the stencils change:
``E(x)(p)`` is the minimum over ``p`` and its 6 face neighbours inside the volume, ``D(x)(p)`` the maximum over the 3 x 3 x 3 window inside the volume;
positions outside the volume never take part -- the published 5-D ``soft_erode`` / ``soft_dilate``: three ``max_pool3d`` of ``(3,1,1)``, ``(1,3,1)``,
``(1,1,3)``, and one of ``(3,3,3)``.  Tie order of the gradient, z slowest: ``E``: z-1, y-1, x-1, centre, x+1, y+1, z+1; ``D``: the 27 offsets with
``dz``, then ``dy``, then ``dx`` ascending.

GRADIENT.  ``relu'(0) = 0``: comparisons are strict.  ``E`` and ``D`` pass the adjoint to the one position they select; among equal values of a window
the first in row-major window order (``E``: up, left, centre, right, down).  When all values of a plane are distinct, every tie inside the
chain traces back to one source position and the gradient does not depend on this rule.  No gradient flows into the target.

CUDA tensors run the HIP kernels of ``csrc/ptb_softskel.hip`` as ONE autograd node (a missing kernel is an error, never torch ops): a tile
kernel with the stencil blocked in time in LDS, a one-workgroup finish, and for the backward the exact adjoint in gather form (no
atomics: the same bits on every run) followed by a streaming pass for the activation.  It keeps the logits, the target and ``ST`` (4 bytes per
position and selected class) instead of the ``4 (k + 1)`` planes autograd keeps of the torch chain.  ``1 <= iterations <= 8`` and at most 32
selected classes run natively; above either cap CUDA tensors raise ``NotImplementedError``.  CPU tensors take the ``max_pool2d`` chain of
``losses/_host.py`` (``max_pool3d`` for volumes): the same definitions, autograd's backward.

With ``dims=3`` CUDA tensors run ``csrc/ptb_softskel3d.hip``, again as ONE autograd node: blocking ``k + 1`` stages in time would need a halo of ``k + 2``
in three axes, so every stage is a launch of its own -- an 8 x 8 x 32 tile with a halo of 2 in LDS, a lane walking a column in z -- and the
levels travel through HBM as fp32.  The backward is a pointwise kernel over the stored ``delta_j``, one gather launch per level (selection
bytes in LDS, no atomics: the same bits on every run) and the same activation pass.  The node keeps the logits, the target, ``ST`` and a
workspace of ``2 (k + 1) + 3`` fp32 values per position and selected class (``v_j+1`` and ``delta_j`` of every stage; the backward reuses the
rest as its scratch and overwrites the deltas, so one backward per forward); under ``torch.no_grad()`` or without a gradient on the
prediction no level is kept (5 values).  A 5-D prediction under the default ``dims=2`` raises ``NotImplementedError``: pass ``dims=3``.

Left out: ``ignore_index``, ``reduction="none"``, anisotropic windows for volumes, more than one stage per launch for volumes, the
pooled-channels form of the paper, a combined Dice + clDice class (add ``DiceLoss`` yourself), a differentiable ``soft_skeleton``, and native
fp16 / bf16 reads (half precision is widened first, like the other losses)."""
from typing import List, Optional

import numpy as np
import torch
from torch import Tensor
from torch.nn.modules.loss import _Loss

from .. import _native as N
from ..utils import softskel as _softskel
from . import _host
from . import _kernels as K
from . import _problem as P

__all__ = ["SoftClDiceLoss", "soft_cldice_loss"]

MAX_CLASSES = 32                                 # SS_MAX_CLASSES of csrc/ptb_softskel.hip


def _check_dims(what, dims):
    if isinstance(dims, bool) or dims not in (2, 3):
        raise ValueError(f"{what}: dims must be 2 or 3, got {dims!r}")
    return int(dims)


def _check_config(what, mode, classes, iterations, smooth):
    P.check_mode(what, mode)
    classes = P.check_classes(what, mode, classes)
    iterations = _softskel.check_iterations(what, iterations)
    smooth = float(smooth)
    if not (smooth >= 0.0 and np.isfinite(smooth)):
        raise ValueError(f"{what}: smooth must be non-negative and finite, got {smooth}")
    return classes, iterations, smooth


class _SoftClDice(torch.autograd.Function):
    """``ptb_soft_cldice_fwd`` / ``ptb_soft_cldice_bwd``.  x fp32 ``[B, C, H, W]``; labels int64 ``[B, H, W]`` or dense fp32 ``[B, C, H, W]``."""

    @staticmethod
    def forward(ctx, x, labels, dense, cls, prob, iterations, smooth):
        B, C, H, W = x.shape
        Kn = len(cls)
        dev = x.device
        classes = N.int_array(cls)
        slots = int(N.load().ptb_soft_cldice_slots(B, Kn, H, W))
        if slots < 0:
            N.check(slots, "soft_cldice_loss")
        ws = torch.empty(4 * slots, dtype=torch.float64, device=dev)
        st = torch.empty((B, Kn, H, W), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty((Kn, 3), dtype=torch.float32, device=dev)
        N.launch("ptb_soft_cldice_fwd", dev, x.data_ptr(), N.ptr(labels), N.ptr(dense), B, C, H, W, classes, Kn, prob, iterations, smooth,
                 st.data_ptr(), ws.data_ptr(), 8 * ws.numel(), loss.data_ptr(), coef.data_ptr(), what="soft_cldice_loss")
        ctx.save_for_backward(x, labels, dense, st, coef)
        ctx.cfg = (cls, prob, iterations)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, labels, dense, st, coef = ctx.saved_tensors
        cls, prob, iterations = ctx.cfg
        B, C, H, W = x.shape
        up = g.to(torch.float32).reshape(1).contiguous()                     # the upstream scalar stays on the device
        dp = torch.empty_like(st)
        grad = torch.empty_like(x)
        N.launch("ptb_soft_cldice_bwd", x.device, x.data_ptr(), N.ptr(labels), N.ptr(dense), B, C, H, W, N.int_array(cls), len(cls), prob, iterations,
                 st.data_ptr(), coef.data_ptr(), up.data_ptr(), dp.data_ptr(), grad.data_ptr(), what="soft_cldice_loss (backward)")
        return grad, None, None, None, None, None, None


class _SoftClDice3d(torch.autograd.Function):
    """``ptb_soft_cldice_3d_fwd`` / ``ptb_soft_cldice_3d_bwd``.  x fp32 ``[B, C, D, H, W]``; labels int64 ``[B, D, H, W]`` or dense fp32 like x.  When a
    gradient is wanted the workspace holds the two level stores and is saved; the backward uses it up, so a second backward raises."""

    @staticmethod
    def forward(ctx, x, labels, dense, cls, prob, iterations, smooth, keep):
        B, C, D, H, W = x.shape
        Kn = len(cls)
        dev = x.device
        keep = int(keep)                                                     # (the caller's grad mode: needs_input_grad does not know torch.no_grad())
        nbytes = int(N.load().ptb_soft_cldice_3d_workspace(B, Kn, D, H, W, iterations, keep))
        if nbytes < 0:
            N.check(nbytes, "soft_cldice_loss")
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        st = torch.empty((B, Kn, D, H, W), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty((Kn, 3), dtype=torch.float32, device=dev)
        N.launch("ptb_soft_cldice_3d_fwd", dev, x.data_ptr(), N.ptr(labels), N.ptr(dense), B, C, D, H, W, N.int_array(cls), Kn, prob, iterations, smooth,
                 keep, st.data_ptr(), ws.data_ptr(), 8 * ws.numel(), loss.data_ptr(), coef.data_ptr(), what="soft_cldice_loss")
        if keep:
            ctx.save_for_backward(x, labels, dense, st, coef, ws)
            ctx.cfg = (cls, prob, iterations)
            ctx.spent = False
        return loss

    @staticmethod
    def backward(ctx, g):
        x, labels, dense, st, coef, ws = ctx.saved_tensors
        cls, prob, iterations = ctx.cfg
        if ctx.spent:
            raise RuntimeError("soft_cldice_loss (backward): dims=3 keeps its levels in a workspace the first backward overwrites, so a second backward "
                               "(retain_graph=True included, unlike dims=2) needs the forward again")
        ctx.spent = True
        B, C, D, H, W = x.shape
        up = g.to(torch.float32).reshape(1).contiguous()                     # the upstream scalar stays on the device
        grad = torch.empty_like(x)
        N.launch("ptb_soft_cldice_3d_bwd", x.device, x.data_ptr(), N.ptr(labels), N.ptr(dense), B, C, D, H, W, N.int_array(cls), len(cls), prob, iterations,
                 st.data_ptr(), coef.data_ptr(), up.data_ptr(), ws.data_ptr(), 8 * ws.numel(), grad.data_ptr(), what="soft_cldice_loss (backward)")
        return grad, None, None, None, None, None, None, None


def soft_cldice_loss(y_pred: Tensor, y_true: Tensor, mode: str, classes: Optional[List[int]] = None, iterations: int = 3, smooth: float = 1.0,
                     from_logits: bool = True, dims: int = 2) -> Tensor:
    """The soft-clDice loss of the module docstring as a 0-dim float32 tensor.  ``y_pred``: ``[B, C, H, W]`` (``dims=3``: ``[B, C, D, H, W]``) in fp32, fp16 or
    bf16 (widened first); ``y_true``: integer labels ``[B, (D,) H, W]`` for ``mode="multiclass"`` (softmax), dense like ``y_pred`` (one channel for
    ``"binary"``) otherwise (sigmoid); ``from_logits=False``: ``y_pred`` already holds probabilities.  ``classes``: the channels that count (default: all)."""
    what = "soft_cldice_loss"
    classes, iterations, smooth = _check_config(what, mode, classes, iterations, smooth)
    dims = _check_dims(what, dims)
    pr = P.problem(what, y_pred, y_true, mode, from_logits, dims=dims, half_or_single=True, exact_labels=True, detach_target=True)
    C, prob = pr.C, pr.prob
    cls = list(range(C)) if classes is None else classes
    if max(cls) >= C:
        raise ValueError(f"{what}: classes {cls} name a channel outside [0, {C})")
    x = pr.x.reshape(pr.B, C, *pr.spatial)                                   # the problem in its planes / volumes again
    labels = None if pr.labels is None else pr.labels.reshape(pr.B, *pr.spatial)
    dense = None if pr.dense is None else pr.dense.reshape(x.shape)
    if not x.is_cuda:
        p = torch.softmax(x, dim=1) if prob == K.PROB_SOFTMAX else torch.sigmoid(x) if prob == K.PROB_SIGMOID else x
        g = dense[:, cls] if labels is None else (labels.unsqueeze(1) == torch.tensor(cls, dtype=torch.int64).reshape(1, -1, *([1] * dims))).to(p.dtype)
        return _host.soft_cldice(p[:, cls], g, iterations, smooth).to(torch.float32)
    if iterations > _softskel.MAX_ITERATIONS:
        raise _softskel.over_cap(what, iterations)
    if len(cls) > MAX_CLASSES:
        raise NotImplementedError(f"{what}: {len(cls)} selected classes; the HIP kernels take at most {MAX_CLASSES} (name fewer in classes=)")
    if dims == 3:                                                            # no level store under torch.no_grad() or without a gradient on the prediction
        return _SoftClDice3d.apply(x, labels, dense, tuple(cls), prob, iterations, smooth, torch.is_grad_enabled() and x.requires_grad)
    return _SoftClDice.apply(x, labels, dense, tuple(cls), prob, iterations, smooth)


class SoftClDiceLoss(_Loss):
    """Soft-clDice loss: ``1 - 2 tprec tsens / (tprec + tsens)`` on soft skeletons of ``iterations`` steps, per selected class and then the mean (the
    module docstring holds the definition, the tie rule of the gradient and what is left out).

    ``mode``: ``"binary"`` (logits ``[B, 1, H, W]``, target of the same size), ``"multiclass"`` (logits ``[B, C, H, W]``, integer labels ``[B, H, W]``,
    softmax) or ``"multilabel"`` (dense targets ``[B, C, H, W]``, sigmoid).  ``classes``: the channels that count (usually the foreground:
    ``classes=[1, ..., C - 1]``).  ``iterations``: the steps of the soft skeleton, about the largest half-width of the structures in
    positions; at most 8 on CUDA tensors.  ``smooth``: added to all four sums.  ``from_logits=False``: ``y_pred`` already holds probabilities.
    ``dims=3``: volumes -- logits ``[B, C, D, H, W]``, labels ``[B, D, H, W]``, ``E`` over the 6 face neighbours and ``D`` over the 3 x 3 x 3 window.
    The published training loss is ``(1 - alpha) DiceLoss + alpha SoftClDiceLoss``; add ``DiceLoss`` yourself."""

    def __init__(self, mode: str, classes: Optional[List[int]] = None, iterations: int = 3, smooth: float = 1.0, from_logits: bool = True,
                 dims: int = 2):
        classes, iterations, smooth = _check_config(type(self).__name__, mode, classes, iterations, smooth)
        dims = _check_dims(type(self).__name__, dims)
        super().__init__()
        self.dims = dims
        self.mode = mode
        self.classes = classes
        self.iterations = iterations
        self.smooth = smooth
        self.from_logits = bool(from_logits)

    def forward(self, y_pred: Tensor, y_true: Tensor) -> Tensor:
        return soft_cldice_loss(y_pred, y_true, self.mode, self.classes, self.iterations, self.smooth, self.from_logits, self.dims)
