"""CPU: the host form of SoftClDiceLoss / soft_skeleton with dims=3 against the float64 max_pool3d chain, and the argument errors."""
import pytest
import torch

import soft_cldice_3d_cases as SC
from pytorch_toolbelt_amd.losses import SoftClDiceLoss, soft_cldice_loss
from pytorch_toolbelt_amd.utils import soft_skeleton


@pytest.mark.parametrize("kind", ("binary", "multiclass", "multilabel", "bf16"))
@pytest.mark.parametrize("k", (1, 3))
def test_host_form_against_the_float64_chain(kind, k):
    y_pred, y_true, mode, kw, leaf, p, g = SC.problem(kind, *SC.SHAPES[0])
    SC.assert_separated(p.detach().flatten(2, 3))
    want = SC.ref_loss(p, g, k)
    want.backward()
    x = y_pred.clone().requires_grad_(True)
    got = SoftClDiceLoss(mode, iterations=k, dims=3, **kw)(x, y_true)
    got.backward()
    assert got.dtype == torch.float32 and got.dim() == 0
    assert abs(float(got.detach()) - float(want.detach())) <= 1e-5
    assert bool(((x.grad.double() - leaf.grad).abs() <= SC.grad_bound(leaf.grad, y_pred.dtype)).all())
    skel = soft_skeleton(p.detach().float(), k, dims=3)
    assert float((skel.double() - SC.ref_skeleton(p.detach().float().double(), k)).abs().max()) <= 4 * (k + 1) * 2.0 ** -24


def test_argument_errors():
    x = torch.zeros(1, 2, 3, 4, 4)
    with pytest.raises(ValueError, match="dims"):
        SoftClDiceLoss("multilabel", dims=4)
    with pytest.raises(ValueError, match="dims"):
        soft_skeleton(x, dims=4)
    with pytest.raises(ValueError):
        soft_cldice_loss(x[0], x[0], "multilabel", dims=3)            # [B, C, H, W] under dims=3
    with pytest.raises(ValueError):
        soft_cldice_loss(x, x, "multilabel", dims=3, classes=[2])
    with pytest.raises(ValueError):
        soft_skeleton(torch.zeros(4, 4), dims=3)
    with pytest.raises(ValueError):
        soft_cldice_loss(x, torch.zeros(1, 4, 4, dtype=torch.int64), "multiclass", dims=3)     # labels [B, H, W]
    with pytest.raises(NotImplementedError, match=r"3-D.*dims=3"):
        soft_cldice_loss(x, x, "multilabel")                          # the default dims=2 keeps refusing 5-D input, and says what to pass
