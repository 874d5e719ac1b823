"""GPU: the distance-map loss kernels (csrc/ptb_distance_loss.hip) against the float64 model of tests/distance_loss_cases.py.

  loss       within seg_loss_cases.TOL (rtol 1e-5) of the model, atol 1e-5 * max(1, mean |term| of the model): the boundary loss cancels
             positive against negative terms, so the absolute bound follows the terms, not the result.
  gradient   within GRAD_TOL (rtol 2e-4), atol 2e-6 * (largest |field value| of the case) * |coef|; on the pixels that hold a logit of +-60
             GRAD_TOL_EXTREME's atol takes the place of the 2e-6.  field = phi (boundary), |phi_pred|^alpha + |phi_truth|^alpha (Hausdorff);
             coef = upstream gradient / count.
  maps       ``class_distance_maps`` has the bits of ``distance_transform(labels, foreground=c, signed=True, ...)`` per class.
  bits       ``dist_maps=`` given, a second run and a chunked run change no bit of loss or gradient.
  calls      the forward makes 2 + chunks native calls (masks, a transform per chunk, the loss), 1 with the boundary loss on ``dist_maps=``."""
import ctypes

import numpy as np
import pytest
import torch

import distance_loss_cases as LC
import seg_loss_cases as SC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd import losses
from pytorch_toolbelt_amd.losses import _kernels as K
from pytorch_toolbelt_amd.utils import class_distance_maps, distance_transform
from pytorch_toolbelt_amd.utils import distance as UD

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FUNCTIONS = {LC.BOUNDARY: losses.boundary_loss, LC.HAUSDORFF: losses.hausdorff_dt_loss}
KINDS = ((LC.BOUNDARY, 2.0), (LC.HAUSDORFF, 2.0))
SWEEP = ([(name, kind, alpha) for name in LC.CASES for kind, alpha in KINDS] + [(name, LC.HAUSDORFF, 1.0) for name in LC.ALPHA_CASES]
         + [(name, LC.HAUSDORFF, 1.5) for name in ("w8", "c9", "spacing")])                # any other alpha: 2^(alpha log2 d)


def _offset(t):
    """a contiguous device copy of ``t`` that starts one element into its buffer: the peeled accesses"""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def _tensors(name):
    case = LC.CASES[name]
    x, t = LC.inputs(name)
    xt = torch.from_numpy(x.copy())
    xt = _offset(xt) if case.offset else xt.to(DEV)
    return case, xt.requires_grad_(True), torch.from_numpy(t.copy()).to(DEV)


def _run(name, kind, alpha=2.0, reduction="mean", **extra):
    """(loss, gradient of loss.sum(), native calls of the forward)"""
    case, x, t = _tensors(name)
    kw = LC.module_arguments(case, kind, alpha, reduction)
    kw.pop("mode")
    kw.update(extra)
    before = N.calls
    loss = FUNCTIONS[kind](x, t, case.mode, **kw)
    calls = N.calls - before
    loss.sum().backward()
    assert N.calls == before + calls + 1, "one native call per backward"
    return loss.detach(), x.grad.detach(), calls


def _check(name, kind, alpha, reduction, loss, grad):
    case = LC.CASES[name]
    want = LC.model(name, kind, alpha, reduction)
    got = loss.cpu().numpy().astype(np.float64)
    assert got.shape == want.loss.shape and loss.dtype == torch.float32
    atol = SC.TOL["atol"] * max(1.0, want.mean_abs_term)
    err = np.abs(got - want.loss)
    print(f"{name} {kind} alpha={alpha} {reduction}: loss {got} model {want.loss} err {err.max():.3e} bound {(SC.TOL['rtol'] * np.abs(want.loss) + atol).min():.3e}")
    assert (err <= SC.TOL["rtol"] * np.abs(want.loss) + atol).all()
    g = grad.cpu().numpy().astype(np.float64)
    x, _ = LC.inputs(name)
    coef = np.abs(want.coef).reshape((-1,) + (1,) * (g.ndim - 1))
    ext = np.broadcast_to(LC.extreme_pixels(case, x), g.shape)
    atol = np.where(ext, SC.GRAD_TOL_EXTREME["atol"], SC.GRAD_TOL["atol"]) * want.field_max * coef
    gerr = np.abs(g - want.grad)
    bound = SC.GRAD_TOL["rtol"] * np.abs(want.grad) + atol
    print(f"    gradient: worst error / bound {np.max(gerr / np.maximum(bound, 1e-300)):.3e}, max |grad| {np.abs(want.grad).max():.3e}")
    assert (gerr <= bound).all()


@pytest.mark.parametrize("name,kind,alpha", SWEEP)
def test_loss_and_gradient_against_the_model(name, kind, alpha):
    loss, grad, calls = _run(name, kind, alpha)
    assert calls == 3, "masks, one transform, the loss"
    _check(name, kind, alpha, "mean", loss, grad)


@pytest.mark.parametrize("kind,alpha", KINDS)
@pytest.mark.parametrize("name", ("w5", "s1025", "c17", "missing", "ignore", "volume", "multilabel_ignore", "spacing"))
def test_per_sample_reduction(name, kind, alpha):
    loss, grad, _ = _run(name, kind, alpha, "none")
    assert loss.shape == (LC.CASES[name].B,)
    _check(name, kind, alpha, "none", loss, grad)


@pytest.mark.parametrize("name", ("w5", "w8", "offset", "missing", "subset_order", "ignore", "volume", "volume_w8", "spacing", "spacing_volume", "s1025"))
def test_class_distance_maps_has_the_bits_of_distance_transform(name):
    case, _, t = _tensors(name)
    dims = len(case.spatial)
    kw = dict(num_classes=case.C, classes=case.classes, dims=dims, spacing=case.spacing, ignore_index=LC.IGNORE if case.ignore else None)
    clean = torch.where(t == LC.IGNORE, torch.full_like(t, -1), t) if case.ignore else t
    for squared in (False, True):
        before = N.calls
        got = class_distance_maps(t, squared=squared, **kw)
        assert N.calls == before + 2, "masks and one transform"
        assert got.shape == (case.B, len(LC.selected(case))) + case.spatial
        for k, c in enumerate(LC.selected(case)):
            want = distance_transform(clean, foreground=c, signed=True, dims=dims, spacing=case.spacing, squared=squared)
            assert got.dtype == want.dtype and torch.equal(got[:, k], want), (k, c, squared)
    host = class_distance_maps(t.cpu(), **kw)
    torch.testing.assert_close(class_distance_maps(t, **kw).cpu(), host, rtol=1e-6, atol=0)


@pytest.mark.parametrize("kind", (LC.BOUNDARY, LC.HAUSDORFF))
@pytest.mark.parametrize("name", ("w5", "subset_order", "missing", "ignore", "volume", "spacing", "spacing_volume"))
def test_given_dist_maps_change_no_bit(name, kind):
    case, _, t = _tensors(name)
    maps = class_distance_maps(t, num_classes=case.C, classes=case.classes, dims=len(case.spatial), spacing=case.spacing,
                               ignore_index=LC.IGNORE if case.ignore else None, squared=case.spacing is None)
    loss, grad, calls = _run(name, kind)
    loss2, grad2, calls2 = _run(name, kind, dist_maps=maps)
    assert calls == 3 and calls2 == (1 if kind == LC.BOUNDARY else 3)          # the boundary loss launches no transform
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    if case.spacing is None:                                                    # float32 distances are accepted as well: the same values
        loss3, grad3, _ = _run(name, kind, dist_maps=class_distance_maps(t, num_classes=case.C, classes=case.classes, dims=len(case.spatial),
                                                                         ignore_index=LC.IGNORE if case.ignore else None))
        torch.testing.assert_close(loss3, loss, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(grad3, grad, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("kind,alpha", KINDS + ((LC.HAUSDORFF, 1.0),))
@pytest.mark.parametrize("name", ("w5", "w8", "s1025", "c9", "c17", "missing", "multilabel", "volume"))
def test_second_run_changes_no_bit(name, kind, alpha):
    for reduction in ("mean", "none"):
        loss, grad, _ = _run(name, kind, alpha, reduction)
        loss2, grad2, _ = _run(name, kind, alpha, reduction)
        assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


@pytest.mark.parametrize("kind", (LC.BOUNDARY, LC.HAUSDORFF))
def test_chunked_run_has_the_bits_of_the_unchunked_one(kind):
    name = LC.CHUNKED
    case = LC.CASES[name]
    planes = 2 if kind == LC.HAUSDORFF else 1
    entries = planes * case.B * 4
    H, W = case.spatial
    whole, _, _ = UD.plan_maps("test", N.load(), 2, case.B, 1, H, W, 4, planes, 4 << 30)
    assert whole == entries
    # S = 42: chunks hold an even number of entries; a cap for three of them leaves chunks of two
    three = ctypes.c_int64()
    assert N.load().ptb_edt_plan(2, 3, 1, H, W, 1, ctypes.byref(three)) == 0
    chunk, _, _ = UD.plan_maps("test", N.load(), 2, case.B, 1, H, W, 4, planes, three.value)
    assert chunk == 2
    loss, grad, calls = _run(name, kind)
    loss2, grad2, calls2 = _run(name, kind, max_workspace_bytes=three.value)
    assert calls == 3 and calls2 == 2 + entries // 2 and entries // 2 >= 2
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    _check(name, kind, 2.0, "mean", loss2, grad2)
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        _run(name, kind, max_workspace_bytes=16)


def test_bad_label_surfaces_through_check_labels():
    case, x, t = _tensors("w8")
    bad = t.clone()
    bad[1, 2, 3] = case.C + 4
    K.flush_label_check()
    for fn in FUNCTIONS.values():
        poisoned = fn(x, bad)
        with pytest.raises(RuntimeError, match="Class values must be smaller"):
            K.flush_label_check()
        assert torch.isnan(poisoned)                                            # never a finite loss from a bad label
        assert torch.isfinite(fn(x, bad, ignore_index=case.C + 4))
        assert torch.isfinite(fn(x, t))
        K.flush_label_check()


@pytest.mark.parametrize("kind", (LC.BOUNDARY, LC.HAUSDORFF))
@pytest.mark.parametrize("name", ("ignore", "ignore_w5", "binary_ignore", "multilabel_ignore"))
def test_ignored_positions_have_exactly_zero_gradient(name, kind):
    case = LC.CASES[name]
    _, t = LC.inputs(name)
    _, grad, _ = _run(name, kind)
    g = grad.cpu().numpy()
    if case.mode == "multiclass":
        ignored = np.broadcast_to((t == LC.IGNORE)[:, None], g.shape)
    else:
        ignored = t == LC.IGNORE
    assert ignored.any() and (g[ignored] == 0).all() and (g[~ignored] != 0).any()


def test_modules_and_half_logits():
    name = "subset"
    case, x, t = _tensors(name)
    for kind, cls in ((LC.BOUNDARY, losses.BoundaryLoss), (LC.HAUSDORFF, losses.HausdorffDTLoss)):
        module = cls(**LC.module_arguments(case, kind))
        loss, _, _ = _run(name, kind)
        assert torch.equal(module(x, t), loss)
        xh = x.detach().half()
        assert torch.equal(module(xh, t), module(xh.float(), t))                # widened first
        host = module(x.detach().cpu(), t.cpu())
        torch.testing.assert_close(loss.cpu(), host, rtol=1e-5, atol=1e-6)
