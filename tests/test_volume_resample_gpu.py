"""GPU: ``resample_volume`` (ptb_volume_resize_trilinear) against the float64 operator model of tests/volume_resample_cases.py.

Tolerance: with d the largest deviation of the float32 numpy restatement from the float64 model on the same input, the kernel stays
within tol = 4 d + 1e-7; float16 / bfloat16 outputs add half an ulp of the output type at the model's value (2^-11 / 2^-8 relative).
torch's CPU ``F.interpolate`` is not the reference here: it evaluates its taps differently and sits up to 7.4e-5 from the model on
these shapes."""
import numpy as np
import pytest
import torch

import volume_resample_cases as VC

pytestmark = pytest.mark.gpu

FLOATS = (torch.float32, torch.float16, torch.bfloat16)
IN_DTYPES = (torch.uint8, torch.int16, torch.uint16, torch.float16, torch.bfloat16, torch.float32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _T():
    from pytorch_toolbelt_amd.inference import tiles_3d

    return tiles_3d


@pytest.mark.parametrize("ac", (False, True), ids=("half-pixel", "align-corners"))
@pytest.mark.parametrize("case", VC.CASES, ids=VC.CASE_IDS)
def test_resample_volume(case, ac, dev):
    """All six input dtypes for [D, H, W] and C in (1, 3, 16), the three output dtypes; integer volumes drawn over the type's full range
    (d scales with the values: up to 8.7e-3 for uint16, where a float16 output overflows to inf beyond 65520 like the model's value
    rounds).  One launch each.  With 16 channels the 4 x 8 x 80 case exceeds the LDS brick too, so both launch forms see every dtype.
    The kernel's float32 error equalled d in every case seen (largest d on N(0, 2) values: 1.1e-6): it gives the restatement's bits,
    the tree is compiled without FMA contraction."""
    from pytorch_toolbelt_amd import _native as N

    extent, size, _ = case
    for k, dtype in enumerate(IN_DTYPES):
        for C in (None, 1, 3, 16):
            v = VC.volume(dtype, tuple(extent) + (() if C is None else (C,)), 100 + k)
            x = v.float().numpy()
            x = x[None] if C is None else np.moveaxis(x, -1, 0)
            model, d, tol = VC.tolerance(x, size, ac)
            vd = v.to(dev)
            for out in FLOATS:
                before = N.calls
                got = _T().resample_volume(vd, size, align_corners=ac, dtype=out)
                assert N.calls == before + 1 and got.dtype == out and got.is_contiguous()
                assert tuple(got.shape) == tuple(size) + (() if C is None else (C,))
                g = got.double().cpu().numpy()
                g = g[None] if C is None else np.moveaxis(g, -1, 0)
                ok, err = VC.within(g, model, tol, out)
                if out == torch.float32 and C in (None, 16):
                    print(f"{dtype} C={C} {extent} -> {size} ac={ac}: d = {d:.3g}, kernel {err:.3g}")
                assert ok, (dtype, C, out, err, tol)


def test_non_contiguous_volume_and_nan(dev):
    """A permuted view is made contiguous first; a NaN reaches exactly the outputs whose taps read it (a lambda = 0 tap included)."""
    v = VC.volume(torch.float32, (9, 10, 11), 5)
    v[4, 5, 6] = float("nan")
    size = (9, 10, 31)
    for ac in (False, True):
        rest = VC.restated_f32(v.numpy()[None], size, ac)[0]
        got = _T().resample_volume(v.to(dev), size, align_corners=ac).cpu().numpy()
        nan = np.isnan(rest)
        assert nan.any() and not nan.all() and np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got[~nan], rest[~nan])
    t = v.to(dev).permute(2, 1, 0)
    assert not t.is_contiguous()
    got = _T().resample_volume(t, (5, 6, 7)).cpu().numpy()
    rest = VC.restated_f32(t.cpu().numpy()[None], (5, 6, 7), False)[0]
    assert np.array_equal(np.isnan(got), np.isnan(rest)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(rest))


def test_resample_volume_refuses(dev):
    T = _T()
    with pytest.raises(NotImplementedError, match="16 channels"):
        T.resample_volume(torch.zeros((2, 2, 2, 17), device=dev), (3, 3, 3))
    with pytest.raises(NotImplementedError):
        T.resample_volume(torch.zeros((2, 2, 2), device=dev, dtype=torch.float64), (3, 3, 3))
    with pytest.raises(ValueError):
        T.resample_volume(torch.zeros((2, 2, 2), device=dev), (3, 3))
    with pytest.raises(RuntimeError, match="requires grad"):
        T.resample_volume(torch.zeros((2, 2, 2), device=dev, requires_grad=True), (3, 3, 3))
