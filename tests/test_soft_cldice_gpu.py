"""GPU: the soft-skeleton kernels (csrc/ptb_softskel.hip) against the float64 chain of soft_cldice_cases.py -- element by element for
soft_skeleton, 1e-5 absolute for the loss (the README's parity line for loss scalars), 1e-5 of the largest reference gradient per element.
bf16 logits run at 5 x 7 only: more positions than that have no distinct equally spaced bf16 logits in [-4, 4]."""
import pytest
import torch

import soft_cldice_cases as SC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.losses import SoftClDiceLoss, soft_cldice_loss
from pytorch_toolbelt_amd.utils import soft_skeleton

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(kind, shape) for kind in ("binary", "multiclass", "multilabel") for shape in SC.SHAPES] + [("bf16", SC.SHAPES[0])]


def run(y_pred, y_true, mode, k, **kw):
    x = y_pred.to(DEV).requires_grad_(True)
    loss = soft_cldice_loss(x, y_true.to(DEV), mode, iterations=k, **kw)
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("k", SC.ITERATIONS)
@pytest.mark.parametrize("shape", SC.SHAPES)
def test_soft_skeleton_per_element(shape, k):
    x = SC.grid_planes(SC.B, *shape, 0, 1, torch.Generator().manual_seed(2)).float()
    want = SC.ref_skeleton(x.double()[:, None], k)[:, 0]
    before = N.calls
    got = soft_skeleton(x.to(DEV), k)
    assert N.calls == before + 1 and got.dtype == torch.float32 and got.shape == x.shape
    err = float((got.cpu().double() - want).abs().max())
    print(f"soft_skeleton {shape} k={k}: max|err| = {err:.3e}")
    assert err <= 4 * (k + 1) * 2.0 ** -24


@pytest.mark.parametrize("k", SC.ITERATIONS)
@pytest.mark.parametrize("kind,shape", CASES)
def test_loss_and_gradient(kind, shape, k):
    y_pred, y_true, mode, kw, leaf, p, g = SC.problem(kind, *shape)
    SC.assert_separated(p.detach())
    want = SC.ref_loss(p, g, k)
    want.backward()
    want = want.detach()
    loss, grad = run(y_pred, y_true, mode, k, **kw)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.dtype == y_pred.dtype
    top = float(leaf.grad.abs().max())
    err = (grad.cpu().double() - leaf.grad).abs()
    print(f"{kind} {shape} k={k}: |loss - ref| = {abs(float(loss) - float(want)):.3e}, max|grad - ref| / max|ref| = {float(err.max()) / top:.3e}")
    assert abs(float(loss) - float(want)) <= 1e-5
    assert bool((err <= SC.grad_bound(leaf.grad, y_pred.dtype)).all())
    host = y_pred.clone().requires_grad_(True)                        # the host form within the same tolerances
    host_loss = soft_cldice_loss(host, y_true, mode, iterations=k, **kw)
    host_loss.backward()
    assert abs(float(loss) - float(host_loss.detach())) <= 1e-5
    assert bool(((grad.cpu().double() - host.grad.double()).abs() <= SC.grad_bound(leaf.grad, y_pred.dtype)).all())


@pytest.mark.parametrize("saturated", (False, True))
def test_two_runs_give_the_same_bits(saturated):
    y_pred, y_true, mode, kw, *_ = SC.problem("multilabel", 45, 83)
    if saturated:                                                     # a 0 / 1 probability plane: the tie rule decides every selection
        y_pred = (y_pred > 0.5).float()
    first, second = run(y_pred, y_true, mode, 3, **kw), run(y_pred, y_true, mode, 3, **kw)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert bool(torch.isfinite(first[1]).all())


def test_above_the_cap():
    x = torch.zeros(1, 1, 8, 8, device=DEV)
    with pytest.raises(NotImplementedError, match=str(SC.CAP)):
        SoftClDiceLoss("binary", iterations=SC.CAP + 1)(x, x)
    with pytest.raises(NotImplementedError, match=str(SC.CAP)):
        soft_skeleton(x, SC.CAP + 1)
    assert N.load().ptb_softskel_cap() == SC.CAP


def test_non_contiguous_prediction_and_a_callers_stream():
    y_pred, y_true, mode, kw, *_ = SC.problem("multiclass", 45, 83)
    want = run(y_pred, y_true, mode, 3, **kw)
    view = y_pred.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)          # channels last
    assert not view.is_contiguous()
    got = run(view, y_true, mode, 3, **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        got = run(y_pred, y_true, mode, 3, **kw)
    stream.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
