"""CPU: the host form of SoftClDiceLoss / soft_skeleton against the float64 chain (loss and gradient), and the argument errors."""
import pytest
import torch

import soft_cldice_cases as SC
from pytorch_toolbelt_amd.losses import SoftClDiceLoss, soft_cldice_loss
from pytorch_toolbelt_amd.utils import soft_skeleton


@pytest.mark.parametrize("kind", ("binary", "multiclass", "multilabel", "bf16"))
@pytest.mark.parametrize("k", (1, 3))
def test_host_form_against_the_float64_chain(kind, k):
    H, W = (5, 7) if kind == "bf16" else (45, 83)
    y_pred, y_true, mode, kw, leaf, p, g = SC.problem(kind, H, W)
    SC.assert_separated(p.detach())
    want = SC.ref_loss(p, g, k)
    want.backward()
    x = y_pred.clone().requires_grad_(True)
    got = SoftClDiceLoss(mode, iterations=k, **kw)(x, y_true)
    got.backward()
    assert got.dtype == torch.float32 and got.dim() == 0
    assert abs(float(got.detach()) - float(want.detach())) <= 1e-5
    assert bool(((x.grad.double() - leaf.grad).abs() <= SC.grad_bound(leaf.grad, y_pred.dtype)).all())


def test_soft_skeleton_host():
    x = SC.grid_planes(3, 13, 9, 0, 1, torch.Generator().manual_seed(1)).float()
    got = soft_skeleton(x, 2)
    assert got.shape == x.shape and got.dtype == torch.float32 and not got.requires_grad
    assert float((got.double() - SC.ref_skeleton(x.double()[:, None], 2)[:, 0]).abs().max()) <= 4 * 3 * 2.0 ** -24
    assert soft_skeleton(torch.zeros(0, 4, 4)).shape == (0, 4, 4)


def test_argument_errors():
    x, y = torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4)
    for bad in ({"mode": "other"}, {"mode": "binary", "classes": [0]}, {"mode": "multilabel", "classes": [0, 0]}, {"mode": "multilabel", "iterations": 0},
                {"mode": "multilabel", "smooth": -1.0}):
        with pytest.raises(ValueError):
            SoftClDiceLoss(**bad)
    with pytest.raises(TypeError):
        SoftClDiceLoss("multilabel", iterations=2.5)
    with pytest.raises(ValueError):
        soft_cldice_loss(x, y, "binary")                              # two channels
    with pytest.raises(ValueError):
        soft_cldice_loss(x, y, "multilabel", classes=[2])
    with pytest.raises(ValueError):
        soft_cldice_loss(x, y, "multiclass")                          # a dense target
    with pytest.raises(ValueError):
        soft_cldice_loss(x, y[:, :1], "multilabel")
    with pytest.raises(TypeError):
        soft_cldice_loss(x.long(), y, "multilabel")
    with pytest.raises(TypeError):
        soft_skeleton(x.double())


def test_volumes_are_refused():
    x = torch.zeros(1, 1, 3, 4, 4)
    with pytest.raises(NotImplementedError, match="3-D"):
        soft_cldice_loss(x, x, "binary")
