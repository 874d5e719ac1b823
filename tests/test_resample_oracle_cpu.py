"""Pins oracle/resample_oracle.py (the float64 operator model the GPU sweep compares the resize kernels with) to ATen on the CPU:
with float64 taps it IS F.interpolate on float64 tensors (forward and autograd gradient, 1e-12); with float32 taps its nearest
modes select the pixels F.interpolate selects on float32 tensors, except at the nearest-exact ties."""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_cases as RC
from oracle import resample_oracle as RO
from oracle import tta_oracle as AO

ALL_SHAPES = RC.SHAPES + [(RC.GRID_STRIDE["other"][1], RC.GRID_STRIDE["other"][2])]
ALL_IDS = RC.SHAPE_IDS + ["grid_stride"]


def _has_exact_tie(n_in, n_out):
    """Some output position's nearest-exact source coordinate (d + 1/2) n_in / n_out is an integer."""
    return any((Fraction(2 * d + 1, 2) * Fraction(n_in, n_out)).denominator == 1 for d in range(n_out))


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=ALL_IDS)
@pytest.mark.parametrize("mode,ac", RC.MODE_CASES, ids=RC.MODE_IDS)
def test_float64_taps_are_aten_float64(mode, ac, shape):
    """Forward and gradient against F.interpolate on float64 CPU tensors, every mode and align_corners, tolerance 1e-12: the operator
    structure (taps, clamps, windows, which index gets which weight) is ATen's."""
    (h, w), size = shape
    x = torch.from_numpy(RC.uniform(RC.PLANES + (h, w), 11).astype(np.float64)).requires_grad_(True)
    ref = F.interpolate(x, size=size, mode=mode, align_corners=ac)
    g = torch.from_numpy(RC.grad_weights(tuple(ref.shape)).astype(np.float64))
    (ref * g).sum().backward()
    out = RO.resize(x.detach().numpy(), size, mode, ac, tap_dtype=np.float64)
    assert out.dtype == np.float64 and out.shape == tuple(ref.shape)
    assert np.abs(out - ref.detach().numpy()).max() <= 1e-12
    gin = RO.resize_adjoint(g.numpy(), (h, w), mode, ac, tap_dtype=np.float64)
    if mode == "nearest-exact" and any(_has_exact_tie(a, b) for a, b in zip((h, w), size)):
        # (2 -> 141: output 70 sits exactly on the pixel boundary.  ATen's forward takes the upper pixel there and its backward kernel
        # the lower one, so autograd is not the adjoint of the forward it differentiates; the model's adjoint is held to the adjoint of
        # ATen's FORWARD instead, whose axis matrices are read off by resizing an identity matrix along one axis)
        Ry = F.interpolate(torch.eye(h, dtype=torch.float64)[None, None], size=(size[0], h), mode=mode)[0, 0]
        Rx = F.interpolate(torch.eye(w, dtype=torch.float64)[None, None], size=(w, size[1]), mode=mode)[0, 0].T
        assert np.abs(gin - (Ry.T @ g @ Rx).numpy()).max() <= 1e-12 * max(1.0, float(x.grad.abs().max()))
    else:
        assert np.abs(gin - x.grad.numpy()).max() <= 1e-12 * max(1.0, float(x.grad.abs().max()))
    # the torch form used for the merges is the same operator, and autograd of it the same adjoint
    xt = x.detach().clone().requires_grad_(True)
    yt = RO.resize_t(xt, size, mode, ac, tap_dtype=np.float64)
    (yt * g).sum().backward()
    assert np.abs(yt.detach().numpy() - out).max() <= 1e-12 and np.abs(xt.grad.numpy() - gin).max() <= 1e-12 * max(1.0, float(x.grad.abs().max()))


def test_float32_taps_nearest_is_aten_on_every_pair_and_nearest_exact_off_the_ties():
    """n_in, n_out in 1..300, one axis, against F.interpolate on float32 CPU tensors.

    'nearest' with float32 taps selects ATen's pixel on all 90 000 pairs.

    'nearest-exact': the float32 product floorf((dst + 0.5f) * scale) and the exact rational index (fractions.Fraction) differ on 1 845
    pairs, always at an exact tie (the rational coordinate is an integer k; the float32 scale lies below n_in / n_out, the product stays
    below k and the rule takes pixel k - 1).  Off that set the model, the rational rule and ATen agree element for element.  Inside
    it CPU ATen follows the float32 rule too, except at 32 pairs (0.04 % of all pairs; the first are 2 -> 141, 2 -> 159, 2 -> 165,
    4 -> 166) where -- only at ties with k = 1 -- it returns the rational rule's pixel.  So the set where ATen differs from the model is
    a subset of the computed tie set, not all of it: CPU ATen is not the rational rule either (300 -> 9 at output 7: rational 250,
    float32 rule and ATen 249).  What the DEVICE kernel of ATen does at these pairs is recorded in
    tests/test_resample_sweep_gpu.py::test_nearest_exact_ties_follow_device_aten."""
    ties = RC.nearest_exact_tie_pairs(300)
    assert {(2, 141), (2, 159), (2, 165), (4, 166)} <= set(ties)
    aten_differs = set()
    for n_in in range(1, 301):
        x = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in, 1)
        for n_out in range(1, 301):
            got = F.interpolate(x, size=(n_out, 1), mode="nearest").flatten().numpy().astype(np.int64)
            assert np.array_equal(got, RO.nearest_index(n_in, n_out, False)), (n_in, n_out)
            got = F.interpolate(x, size=(n_out, 1), mode="nearest-exact").flatten().numpy().astype(np.int64)
            model = RO.nearest_index(n_in, n_out, True)
            if not np.array_equal(got, model):
                aten_differs.add((n_in, n_out))
                pos = np.nonzero(got != model)[0]
                assert (n_in, n_out) in ties and set(pos) <= set(ties[(n_in, n_out)]), (n_in, n_out)
                assert np.array_equal(got[pos], RO.nearest_exact_index_rational(n_in, n_out)[pos]), (n_in, n_out)
    print("nearest-exact: tie pairs", len(ties), "pairs where CPU ATen differs from the float32 rule", len(aten_differs))
    assert 0 < len(aten_differs) <= 90          # 0.1 % of the pairs
    assert {(2, 141), (2, 159), (2, 165), (4, 166)} <= aten_differs


@pytest.mark.parametrize("mode,ac", RC.MODE_CASES, ids=RC.MODE_IDS)
def test_float32_taps_stay_next_to_the_float32_restatement(mode, ac):
    """The model with float32 taps against oracle.tta_oracle in float32 on the sweep's shapes: nearest modes select the same pixels
    (deviation 0); the interpolating modes differ by float32 rounding of the sums only (measured here: bilinear 1.1e-7, bicubic 2.2e-7,
    area 2.0e-7 -- the bounds are a few ulp of values below 1.3 (bicubic overshoots) times the taps summed; area: n 2^-24 for
    the largest window, the 35 pixels of 5 x 7 -> 1 x 1)."""
    bound = {"nearest": 0.0, "nearest-exact": 0.0, "bilinear": 4 * 2.0 ** -23, "bicubic": 16 * 2.0 ** -23, "area": 35 * 2.0 ** -24}[mode]
    worst = 0.0
    for (h, w), size in RC.SHAPES:
        x = RC.uniform(RC.PLANES + (h, w), 5)
        worst = max(worst, float(np.abs(AO._resize(x, size, mode, ac).astype(np.float64) - RO.resize(x, size, mode, ac)).max()))
    print(mode, ac, "deviation of the float32 restatement", worst)
    assert worst <= bound


def test_vectorised_area_is_the_loop():
    for (h, w), size in RC.SHAPES:
        x = RC.uniform(RC.PLANES + (h, w), 6)
        assert np.array_equal(RO.area_resize_f32(x, size), AO.area_resize(x, size))


@pytest.mark.parametrize("reduction", RO.REDUCTIONS)
def test_merge_model_is_the_restated_merge(reduction):
    """ms_merge_t (float64 taps) against F.interpolate + the reference's reductions restated in float64 torch, and (float32 taps)
    next to oracle.tta_oracle.ms_image_deaugment in float32."""
    size = (36, 52)
    srcs = [(12, 20), (36, 52), (108, 156)]
    maps = [RC.uniform((2, 2) + s, 20 + i) for i, s in enumerate(srcs)]
    t64 = [torch.from_numpy(m.astype(np.float64)) for m in maps]
    for ac in (False, True):
        back = torch.stack([m if tuple(m.shape[-2:]) == size else F.interpolate(m, size=size, mode="bilinear", align_corners=ac) for m in t64])
        ref = AO.deaugment_averaging(back.numpy(), reduction)           # the numpy restatement, evaluated in float64
        got = RO.ms_merge_t(t64, size, reduction, ac, tap_dtype=np.float64).numpy()
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
        f32 = AO.ms_image_deaugment(maps, RC.offsets_for(srcs, size), reduction, ac)
        np.testing.assert_allclose(f32, RO.ms_merge_t(t64, size, reduction, ac).numpy(), rtol=1e-5, atol=1e-6)


def test_merge_model_unflips_views():
    size = (8, 12)
    views = (0, 4, 2, 6)                     # d2: identity, fliplr, flipud, rot180
    y = torch.from_numpy(RC.uniform((4 * 2, 3, 8, 12), 9).astype(np.float64))
    got = RO.ms_merge_t([y], size, "mean", True, views=views, inner="gmean").numpy()
    ref = AO.image_deaugment(y.numpy(), "d2", "gmean")
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
