"""The soft skeleton of probability maps (Shit et al., CVPR 2021: the ``soft_skel`` of clDice) on the device the tensor is on::

    skel = soft_skeleton(probabilities, iterations=3)          # float32 [*stack, H, W] -> the same shape
    skel = soft_skeleton(volumes, iterations=3, dims=3)        # float32 [*stack, D, H, W]: 6 face neighbours, 3 x 3 x 3 windows

``losses/cldice.py`` holds the definition (``v_j+1 = E(v_j)``, ``delta_j = relu(v_j - D(v_j+1))``, ``S_j = S_j-1 + relu(delta_j - S_j-1 delta_j)``) and the
training loss built on it, for planes and for volumes.  This function is the forward tile kernel of ``csrc/ptb_softskel.hip`` alone
(``dims=3``: the stage kernel of ``csrc/ptb_softskel3d.hip``, one launch per stage): it returns no graph (a differentiable soft skeleton
is left out; train through ``SoftClDiceLoss``).  CUDA tensors run those kernels -- a missing kernel is an error --, CPU tensors the
``max_pool2d`` / ``max_pool3d`` chain of ``losses/_host.py``."""
import torch

from .. import _native as N
from . import _maps as M

__all__ = ["soft_skeleton"]

MAX_ITERATIONS = 8                               # SS_CAP of csrc/ptb_softskel.hip, the library's ptb_softskel_cap()


def check_iterations(what, iterations):
    iterations = M.check_int(what, "iterations", iterations)
    if iterations < 1:
        raise ValueError(f"{what}: iterations must be at least 1, got {iterations}")
    return iterations


def over_cap(what, iterations):
    return NotImplementedError(f"{what}: iterations={iterations} is above the cap of {MAX_ITERATIONS} the HIP kernels hold in LDS (CUDA tensors take no torch ops)")


def soft_skeleton(x, iterations=3, dims=2):
    """``softskel_iterations`` of every ``H x W`` plane of the float32 tensor ``x [*stack, H, W]`` (values in ``[0, 1]``), as a new float32 tensor of the
    same shape, detached; with ``dims=3`` of every ``D x H x W`` volume of ``x [*stack, D, H, W]``.  CUDA tensors, ``dims=2``: ONE launch on the current
    stream, a workgroup per 32 x 32 tile with a halo of ``iterations + 2`` in LDS; ``dims=3``: one native call of ``iterations + 1`` launches, a
    workgroup per 8 x 8 x 32 tile with a halo of 2, two rolling fp32 levels in a workspace of twice the input.  Nothing is read back;
    ``1 <= iterations <= 8``, above that ``NotImplementedError``.  Empty inputs return without a launch."""
    what = "soft_skeleton"
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise TypeError(f"{what}: x must be a float32 tensor, got {getattr(x, 'dtype', type(x))}")
    iterations = check_iterations(what, iterations)
    _, B, D, H, W = M.extent(what, "x", x, dims)
    if B * D * H * W == 0:
        return torch.empty_like(x)
    x = x.detach()
    if not x.is_cuda:
        from ..losses import _host

        return _host.soft_skeleton(x.reshape((B, 1, D, H, W) if dims == 3 else (B, 1, H, W)), iterations).reshape(x.shape)
    if iterations > MAX_ITERATIONS:
        raise over_cap(what, iterations)
    x = x.contiguous()
    out = torch.empty_like(x)
    if dims == 3:
        ws = torch.empty(2 * x.numel(), dtype=torch.float32, device=x.device)
        N.launch("ptb_soft_skeleton_3d", x.device, x.data_ptr(), B, D, H, W, iterations, out.data_ptr(), ws.data_ptr(), 4 * ws.numel(), what=what)
    else:
        N.launch("ptb_soft_skeleton", x.device, x.data_ptr(), B, H, W, iterations, out.data_ptr(), what=what)
    return out
