"""The arms of the host-side kernel dispatch (csrc/ptb_dispatch.h) at the smallest shapes that still select them, against the
oracles and at the tolerances of the neighbouring suites (tests/test_tiles_gpu.py: 1e-5 absolute for the fused TTA merge;
tests/test_losses_gpu.py: 1e-5 absolute against the fp64 oracle, 2e-6 relative between the straight-line and the generic kernels).

View families: 32 x 32 tiles with 16 pixels of overlap, every view set that has a compiled-in instance, fp32 / fp16 / bf16
sources, a linear and a non-linear reduction, incremental / planned / deferred mergers, both settings of
ptb_set_tunable(1, .).  Loss families: C on both sides of the 4 / 8 / 16 register buckets, HW = 256 and 1024 (straight-line and packed
kernels eligible) and 252 (not eligible).  Volume families: 8 x 8 x 8 tiles, every mirror set, the three source types, a linear and a
non-linear reduction, both settings of the tunable (tests/test_volume_tta_gpu.py: torch's stack reduction, 1e-6 / 1e-5 for fp32, one
rounding to the source type otherwise)."""
import numpy as np
import pytest
import torch

from oracle import losses_oracle as LO
from oracle import tiles_oracle as TO
from oracle import tta_oracle as AO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def lib():
    from pytorch_toolbelt_amd import _native as N

    lib = N.load()
    yield lib
    lib.ptb_set_tunable(1, 0)


# ------------------------------------------------------------------ view sets x source dtype x reduction
GROUPS = {"fliplr": 2, "flipud": 2, "flips": 3, "d2": 4, "d4": 8}
GEOM = TO.slicer_geometry((80, 64), (32, 32), (16, 16))
WINDOW = TO.pyramid_window(32, 32)[0]
_want = {}


def _view_case(group, reduction, dtype):
    """Seeded chunk-major model outputs of every tile (values a half type holds exactly) and the oracle's merged map, computed once."""
    key = (group, reduction, dtype)
    if key not in _want:
        V, n, C = GROUPS[group], len(GEOM["crops"]), 2
        rng = np.random.default_rng(11)
        x = torch.from_numpy((rng.random((V * n, C, 32, 32)) * 0.9 + 0.05).astype(np.float32)).to(dtype)
        st = TO.merger_new(GEOM["target_shape"], C, WINDOW)
        TO.merger_integrate(st, AO.image_deaugment(x.float().numpy(), group, reduction), GEOM["crops"])
        _want[key] = (x, TO.merger_merge(st))
    return _want[key]


@pytest.mark.parametrize("scalar", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("reduction", ["mean", "gmean"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_view_sets_and_source_dtypes(group, reduction, dtype, scalar, dev, lib):
    from pytorch_toolbelt_amd.inference.tiles import TileMerger

    x, want = _view_case(group, reduction, dtype)
    crops, C = GEOM["crops"], 2
    lib.ptb_set_tunable(1, scalar)
    # (the planned and deferred mergers are built on the 16-byte kernels: with those switched off the incremental merger is the case)
    for kw in ((dict(), dict(crops=crops), dict(crops=crops, defer=True)) if not scalar else (dict(),)):
        m = TileMerger(GEOM["target_shape"], C, WINDOW, device=dev, **kw)
        m.integrate_batch_deaugment(x.to(dev), crops, group=group, reduction=reduction)
        np.testing.assert_allclose(m.merge().cpu().numpy(), want, rtol=0, atol=1e-5, err_msg=str(kw))


# ------------------------------------------------------------------ class buckets x HW eligibility
@pytest.mark.parametrize("hw", [(16, 16), (32, 32), (14, 18)], ids=["HW256", "HW1024", "HW252"])
@pytest.mark.parametrize("C", [3, 4, 5, 8, 9, 16, 17])
def test_loss_class_buckets(C, hw, dev, lib):
    from pytorch_toolbelt_amd import losses as L

    g = torch.Generator().manual_seed(1000 + C)
    B = 2
    logits = torch.randn((B, C, *hw), generator=g) * 2.5
    labels = torch.randint(0, C, (B, *hw), generator=g)
    x64, l64 = logits.numpy(), labels.numpy()
    xl, ll = logits.to(dev), labels.to(dev)
    want = (LO.dice_loss(x64, l64, "multiclass", smooth=0.5), LO.jaccard_loss(x64, l64, "multiclass"),
            LO.binary_focal_loss(x64, l64) + LO.dice_loss(x64, l64, "multiclass") + LO.jaccard_loss(x64, l64, "multiclass"),
            float(LO.softmax_focal_loss_with_logits(x64, l64)), LO.binary_focal_loss(x64, l64))
    results, grads = [], []
    for scalar in (0, 1):
        lib.ptb_set_tunable(1, scalar)
        try:
            xg = xl.clone().requires_grad_(True)
            fused = L.FocalDiceJaccardLoss("multiclass")(xg, ll)
            fused.backward()
            results.append((float(L.DiceLoss("multiclass", smooth=0.5)(xl, ll)), float(L.JaccardLoss("multiclass")(xl, ll)), float(fused),
                            float(L.CrossEntropyFocalLoss()(xl, ll)), float(L.BinaryFocalLoss()(xl, ll))))
            grads.append(xg.grad)
        finally:
            lib.ptb_set_tunable(1, 0)
    print(C, hw, results[0], want)
    assert results[0] == pytest.approx(results[1], rel=2e-6, abs=1e-6)
    torch.testing.assert_close(grads[0], grads[1], rtol=5e-5, atol=1e-9)
    assert results[0] == pytest.approx(want, abs=1e-5)


# ------------------------------------------------------------------ 3-D mirror sets x source dtype x reduction
FLIPS = {0: [], 1: [4], 2: [3], 3: [3, 4], 4: [2], 5: [2, 4], 6: [2, 3], 7: [2, 3, 4]}
VOLUME_REDUCTIONS = {"mean": (lambda s: s.mean(0), 1e-6), "gmean": (lambda s: s.log().mean(0).exp(), 1e-5)}


@pytest.mark.parametrize("scalar", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("reduction", list(VOLUME_REDUCTIONS))
def test_volume_mirror_sets_and_source_dtypes(reduction, dtype, scalar, dev, lib):
    from pytorch_toolbelt_amd.inference import MIRROR_VIEWS, mirror_volume_deaugment

    red, tol = VOLUME_REDUCTIONS[reduction]
    g = torch.Generator().manual_seed(21)
    lib.ptb_set_tunable(1, scalar)
    for mirror, views in MIRROR_VIEWS.items():
        y = (torch.rand((len(views) * 2, 2, 8, 8, 8), generator=g) * 0.98 + 0.01).to(dtype).to(dev)
        want = red(torch.stack([c.flip(FLIPS[m]) if FLIPS[m] else c for c, m in zip(y.float().chunk(len(views)), views)]))
        got = mirror_volume_deaugment(y, mirror, reduction)
        assert got.dtype == dtype
        if dtype == torch.float32:
            torch.testing.assert_close(got, want, rtol=tol, atol=tol, msg=mirror)
        else:
            torch.testing.assert_close(got, want.to(dtype), msg=mirror)    # one rounding to the source type
