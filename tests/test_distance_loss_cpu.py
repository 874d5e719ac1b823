"""CPU: the host form of the distance-map losses (losses/distance_losses.py) and of ``utils.class_distance_maps`` against the float64
model and scipy restatement of tests/distance_loss_cases.py, the argument validation of the native entry points (which returns before any
launch), the constructors' errors and the exports."""
import ctypes

import numpy as np
import pytest
import torch

import distance_loss_cases as LC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd import losses, utils
from pytorch_toolbelt_amd.losses import distance_losses as DL
from pytorch_toolbelt_amd.utils import distance as UD

# the host form is float32 torch algebra on float64-derived maps: the bound of the device form serves
RTOL, ATOL = 1e-5, 1e-5
FUNCTIONS = {LC.BOUNDARY: losses.boundary_loss, LC.HAUSDORFF: losses.hausdorff_dt_loss}
HOST_CASES = ("w5", "c1", "c5", "c17", "missing", "subset", "subset_order", "ignore", "volume", "spacing", "spacing_volume", "binary", "binary_ignore",
              "multilabel", "multilabel_subset", "multilabel_ignore", "probabilities", "probabilities_binary", "extreme")


def _call(name, kind, alpha, reduction, dist_maps=None):
    case = LC.CASES[name]
    x, t = LC.inputs(name)
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    kw = LC.module_arguments(case, kind, alpha, reduction)
    kw.pop("mode")
    loss = FUNCTIONS[kind](xt, torch.from_numpy(t.copy()), case.mode, dist_maps=dist_maps, **kw)
    return xt, loss


@pytest.mark.parametrize("reduction", ("mean", "none"))
@pytest.mark.parametrize("kind,alpha", ((LC.BOUNDARY, 2.0), (LC.HAUSDORFF, 2.0), (LC.HAUSDORFF, 1.0)))
@pytest.mark.parametrize("name", HOST_CASES)
def test_host_form_against_the_model(name, kind, alpha, reduction):
    want = LC.model(name, kind, alpha, reduction)
    xt, loss = _call(name, kind, alpha, reduction)
    assert loss.shape == want.loss.shape and loss.dtype == torch.float32
    np.testing.assert_allclose(loss.detach().numpy(), want.loss, rtol=RTOL, atol=ATOL * max(1.0, want.mean_abs_term))
    loss.sum().backward()
    scale = want.field_max * float(np.abs(want.coef).max())
    np.testing.assert_allclose(xt.grad.numpy(), want.grad, rtol=2e-4, atol=(1e-4 if LC.CASES[name].extreme else 2e-6) * max(scale, 1e-30))


@pytest.mark.parametrize("name", ("w5", "missing", "subset_order", "ignore", "volume", "spacing", "spacing_volume"))
def test_class_distance_maps_host_form_against_scipy(name):
    case = LC.CASES[name]
    _, t = LC.inputs(name)
    dims = len(case.spatial)
    cls = LC.selected(case)
    objects = t[:, None] == np.asarray(cls).reshape((1, -1) + (1,) * dims)
    kw = dict(num_classes=case.C, classes=case.classes, dims=dims, spacing=case.spacing, ignore_index=LC.IGNORE if case.ignore else None)
    got = utils.class_distance_maps(torch.from_numpy(t.copy()), **kw)
    assert got.shape == (case.B, len(cls)) + case.spatial and got.dtype == torch.float32
    want = LC.signed_maps(objects, dims, case.spacing)
    np.testing.assert_allclose(got.numpy(), want.astype(np.float32), rtol=2e-7 if case.spacing is None else 1e-6)
    if case.spacing is None:
        sq = utils.class_distance_maps(torch.from_numpy(t.copy()), squared=True, **kw)
        assert sq.dtype == torch.int32 and np.array_equal(sq.numpy(), LC.signed_squared(objects, dims))
        for k, c in enumerate(cls):                         # the documented identity with distance_transform
            one = utils.distance_transform(torch.from_numpy(np.where(t == LC.IGNORE, -1, t) if case.ignore else t.copy()), foreground=c, signed=True,
                                           dims=dims)
            assert torch.equal(got[:, k], one)
    if name == "missing":                                   # the infinities stay in the maps
        assert np.isposinf(got.numpy()[0, 1]).all() and np.isneginf(got.numpy()[1, 1]).all() and np.isposinf(got.numpy()[1, 0]).all()


def test_host_form_takes_dist_maps():
    for name, squared in (("subset_order", True), ("subset_order", False), ("spacing", False)):
        case = LC.CASES[name]
        _, t = LC.inputs(name)
        maps = utils.class_distance_maps(torch.from_numpy(t.copy()), num_classes=case.C, classes=case.classes, spacing=case.spacing, squared=squared)
        for kind in (LC.BOUNDARY, LC.HAUSDORFF):
            xa, a = _call(name, kind, 2.0, "mean")
            xb, b = _call(name, kind, 2.0, "mean", dist_maps=maps)
            np.testing.assert_allclose(b.item(), a.item(), rtol=1e-6)
            a.backward()
            b.backward()
            np.testing.assert_allclose(xb.grad.numpy(), xa.grad.numpy(), rtol=1e-5, atol=1e-9)


def test_modules_are_the_functions():
    name = "subset"
    case = LC.CASES[name]
    x, t = LC.inputs(name)
    for kind, cls in ((LC.BOUNDARY, losses.BoundaryLoss), (LC.HAUSDORFF, losses.HausdorffDTLoss)):
        module = cls(**LC.module_arguments(case, kind, 2.0, "none"))
        got = module(torch.from_numpy(x.copy()), torch.from_numpy(t.copy()))
        _, want = _call(name, kind, 2.0, "none")
        assert got.shape == (case.B,) and torch.equal(got, want.detach())
    xh = torch.from_numpy(x.copy()).half()                  # fp16 / bf16 logits are widened first
    half = losses.BoundaryLoss("multiclass")(xh, torch.from_numpy(t.copy()))
    assert half.dtype == torch.float32 and torch.equal(half, losses.BoundaryLoss("multiclass")(xh.float(), torch.from_numpy(t.copy())))


# ---------------------------------------------------------------------------------------------------------------- native validation
def _plan(*args):
    out = [ctypes.c_int64() for _ in range(4)]
    rc = N.load().ptb_dloss_plan(*args, *[ctypes.byref(o) for o in out])
    return rc, [o.value for o in out]


def test_plan_without_gpu():
    rc, (chunk, nbytes, least, slots) = _plan(2, 2, 1, 6, 7, 4, 2, 4 << 30)
    assert rc == 0 and chunk == 16 and slots == 2 and least <= nbytes
    edt = ctypes.c_int64()
    assert N.load().ptb_edt_plan(2, 16, 1, 6, 7, 1, ctypes.byref(edt)) == 0 and nbytes == edt.value
    # a cap for fewer entries: S = 42 is even, not a multiple of 4: chunks of an even number of entries, each output 16-byte aligned
    assert N.load().ptb_edt_plan(2, 7, 1, 6, 7, 1, ctypes.byref(edt)) == 0
    rc, (chunk, nbytes, _, _) = _plan(2, 2, 1, 6, 7, 4, 2, edt.value)
    assert rc == 0 and chunk == 6 and nbytes <= edt.value
    rc, (_, _, least2, _) = _plan(2, 2, 1, 6, 7, 4, 2, least - 1)
    assert rc == -1 and least2 == least
    assert _plan(2, 2, 1, 5, 5, 4, 1, 1300)[1][0] == 4                         # S odd: multiples of four entries (five would fit the cap)
    assert _plan(2, 3, 1, 16, 64, 2, 1, 4 << 30)[1][3] == 3 and _plan(2, 3, 1, 16, 65, 2, 1, 4 << 30)[1][3] == 6      # B * ceil(S / 1024) slots
    for bad in ((4, 2, 1, 6, 7, 4, 2, 1 << 30), (2, 0, 1, 6, 7, 4, 2, 1 << 30), (2, 2, 1, 6, 7, 0, 2, 1 << 30), (2, 2, 1, 6, 7, 4, 3, 1 << 30),
                (2, 2, 2, 6, 7, 4, 2, 1 << 30), (2, 2, 1, 6, 7, 4, 2, -1)):
        assert _plan(*bad)[0] == -1, bad
    assert _plan(2, 1, 1, 1 << 16, 1 << 16, 1, 1, 1 << 40)[0] == N.PTB_EUNSUPPORTED      # a sample past 2^31 - 2 positions


def test_argument_validation_without_gpu():
    """Every refusal below returns before the first launch, so the pointers are never followed: any non-null value serves."""
    lib = N.load()
    P = 1 << 20                                             # stands for a device pointer, 16-byte aligned
    cls = N.int_array([1, 3])
    B, C, K, S = 2, 4, 2, 48

    def masks(**kw):
        a = dict(logits=P, labels=P, dense=None, classes=cls, table=P, planes=3, B=B, C=C, K=K, S=S, prob=0, masks=P)
        a.update(kw)
        return lib.ptb_dloss_masks(a["logits"], a["labels"], a["dense"], a["classes"], a["table"], a["planes"], a["B"], a["C"], a["K"], a["S"], a["prob"],
                                   0, 0, 0.0, a["masks"], None)

    def fwd(kind=1, **kw):
        a = dict(logits=P, labels=P, dense=None, classes=cls, table=P, truth=P, pred=P, maps_kind=0, B=B, C=C, K=K, S=S, prob=0, alpha=2.0, ws=P,
                 ws_bytes=1 << 20, loss=P, inv=P, flag=P)
        a.update(kw)
        return lib.ptb_dloss_fwd(kind, a["logits"], a["labels"], a["dense"], a["classes"], a["table"], a["truth"], a["pred"], a["maps_kind"], a["B"], a["C"],
                                 a["K"], a["S"], a["prob"], 0, 0, 0.0, a["alpha"], 0, a["ws"], a["ws_bytes"], a["loss"], a["inv"], a["flag"], None)

    def bwd(kind=1, **kw):
        a = dict(logits=P, labels=P, dense=None, classes=cls, table=P, truth=P, pred=P, maps_kind=0, B=B, C=C, K=K, S=S, prob=0, alpha=2.0, coef=P, grad=P)
        a.update(kw)
        return lib.ptb_dloss_bwd(kind, a["logits"], a["labels"], a["dense"], a["classes"], a["table"], a["truth"], a["pred"], a["maps_kind"], a["B"], a["C"],
                                 a["K"], a["S"], a["prob"], 0, 0, 0.0, a["alpha"], 0, a["coef"], a["grad"], None)

    common = (dict(logits=None), dict(labels=None), dict(dense=P), dict(K=0), dict(K=5, classes=N.int_array([0, 1, 2, 3, 3])), dict(B=0), dict(C=0), dict(S=0),
              dict(classes=N.int_array([1, 4])), dict(classes=N.int_array([-1, 2])), dict(classes=N.int_array([2, 2])), dict(classes=None),
              dict(table=None), dict(classes=None, table=None), dict(prob=3))
    for kw in common:
        assert masks(**kw) == -1, kw
        assert fwd(**kw) == -1, kw
        assert bwd(**kw) == -1, kw
    for kw in (dict(masks=None), dict(planes=0), dict(planes=4)):
        assert masks(**kw) == -1, kw
    for kw in (dict(truth=None), dict(pred=None), dict(kind=0), dict(kind=2), dict(maps_kind=2), dict(alpha=0.0), dict(alpha=float("inf"))):
        assert fwd(**kw) == -1, kw
        assert bwd(**kw) == -1, kw
    for kw in (dict(ws=None), dict(ws=P + 8), dict(ws_bytes=16 * B - 1), dict(loss=None), dict(inv=None), dict(flag=None)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(coef=None), dict(grad=None)):
        assert bwd(**kw) == -1, kw
    assert fwd(S=1 << 31) == N.PTB_EUNSUPPORTED and masks(S=1 << 31) == N.PTB_EUNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- python errors
def test_constructor_and_call_errors():
    for cls in (losses.BoundaryLoss, losses.HausdorffDTLoss):
        with pytest.raises(ValueError, match="mode"):
            cls("panoptic")
        with pytest.raises(ValueError, match="binary"):
            cls("binary", classes=[0])
        with pytest.raises(ValueError, match="reduction"):
            cls("multiclass", reduction="sum")
        with pytest.raises(ValueError, match="classes"):
            cls("multiclass", classes=[1, 1])
        with pytest.raises(ValueError, match="spacing"):
            cls("multiclass", spacing=(1.0, -2.0))
    with pytest.raises(ValueError, match="alpha"):
        losses.HausdorffDTLoss("multiclass", alpha=0.0)
    with pytest.raises(TypeError):
        losses.BoundaryLoss("multiclass", alpha=1.0)
    x, t = torch.zeros(2, 3, 4, 5), torch.zeros(2, 4, 5, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        losses.boundary_loss(x[0], t)
    with pytest.raises(ValueError, match="classes"):
        losses.boundary_loss(x, t, classes=[3])
    with pytest.raises(ValueError, match="integer labels"):
        losses.boundary_loss(x, t.float())
    with pytest.raises(ValueError, match="spacing"):
        losses.boundary_loss(x, t, spacing=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="does not match"):
        losses.boundary_loss(x, torch.zeros(2, 3, 4, 4), "multilabel")
    with pytest.raises(ValueError, match="one channel"):
        losses.boundary_loss(x, torch.zeros(2, 3, 4, 5), "binary")
    with pytest.raises(ValueError, match="dist_maps"):
        losses.boundary_loss(x, t, dist_maps=torch.zeros(2, 2, 4, 5))
    with pytest.raises(TypeError, match="dist_maps"):
        losses.boundary_loss(x, t, dist_maps=torch.zeros(2, 3, 4, 5, dtype=torch.float64))
    with pytest.raises(TypeError, match="dist_maps"):
        losses.boundary_loss(x, t, spacing=(1.0, 2.0), dist_maps=torch.zeros(2, 3, 4, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match="num_classes"):
        utils.class_distance_maps(t)
    with pytest.raises(ValueError, match=r"\[B, H, W\]"):
        utils.class_distance_maps(t[0], num_classes=3)
    with pytest.raises(TypeError, match="integer"):
        utils.class_distance_maps(t.float(), num_classes=3)
    with pytest.raises(ValueError, match="classes"):
        utils.class_distance_maps(t, num_classes=3, classes=[0, 3])
    assert utils.class_distance_maps(t[:0], num_classes=3).shape == (0, 3, 4, 5)
    assert utils.class_distance_maps(t, classes=[2, 0]).shape == (2, 2, 4, 5)


def test_exports():
    assert DL.__all__ == ["BoundaryLoss", "HausdorffDTLoss", "boundary_loss", "hausdorff_dt_loss"]
    for name in DL.__all__:
        assert getattr(losses, name) is getattr(DL, name)
    assert utils.class_distance_maps is UD.class_distance_maps and "class_distance_maps" in UD.__all__
    for name in ("ptb_dloss_plan", "ptb_dloss_masks", "ptb_dloss_fwd", "ptb_dloss_bwd"):
        assert name in N.SIGNATURES and hasattr(N.load(), name)
