"""CPU: the host form of ``surface_metrics`` (utils/surface.py) against the scipy yardstick of tests/surface_cases.py, the yardstick
against an all-pairs brute force, every validation error and the conventions for empty surfaces.

  counts, surface Dice          equal integers: surface Dice must be float32(within / total) of the yardstick's counts, bit for bit
  Hausdorff, unit spacing       float32(sqrt(float64(exact squared integer))), bit for bit
  percentiles, means, assd      rtol 1e-6 with unit spacing, 2e-6 with spacing (the bounds of the device tests; the host form is float64
                                until its one rounding to float32, 6e-8)
``inf`` / ``nan`` exactly where the yardstick has them."""
import math

import numpy as np
import pytest
import torch

import surface_cases as SC
from pytorch_toolbelt_amd.utils import surface_metrics

def check(name, got, want, spacing, what):
    """a result dict of ``surface_metrics`` (tensors, any device) against ``SC.expected``"""
    case = SC.CASES[name]
    stack = case.pred.shape[:-case.dims]
    K = 1 if case.labels is None else len(case.labels)
    rtol = 1e-6 if spacing is None else 2e-6
    assert set(got) == {"surface_count", "surface_dice", *SC.KEYS1, *SC.KEYS2}, what
    g = {k: v.cpu().numpy().reshape((-1, K) + tuple(v.shape[len(stack) + 1:])) for k, v in got.items()}
    for k, v in got.items():
        tail = (K, 2) if k in SC.KEYS2 + ("surface_count",) else (K, len(SC.TOLERANCES)) if k == "surface_dice" else (K,)
        assert tuple(v.shape) == stack + tail and v.dtype == (torch.int64 if k == "surface_count" else torch.float32), (what, k, v.shape, v.dtype)
    assert np.array_equal(g["surface_count"], want["surface_count"]), what
    total = want["surface_count"].sum(axis=-1, keepdims=True).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        dice = np.where(total > 0, want["within"] / total, np.nan).astype(np.float32)
    assert np.array_equal(g["surface_dice"], dice, equal_nan=True), (what, "surface_dice", g["surface_dice"], dice)
    if spacing is None:
        sq = want["max_squared"]
        exact = np.where(sq >= 0, np.sqrt(np.maximum(sq, 0).astype(np.float64)), want["directed_hausdorff"]).astype(np.float32)
        assert np.array_equal(g["directed_hausdorff"], exact, equal_nan=True), (what, "directed_hausdorff")
        both = np.where(np.isfinite(want["hausdorff"]), exact.max(axis=-1), want["hausdorff"].astype(np.float32))
        assert np.array_equal(g["hausdorff"], both, equal_nan=True), (what, "hausdorff")
    for k in SC.KEYS1 + SC.KEYS2:
        a, w = g[k].astype(np.float64), want[k]
        fin = np.isfinite(w)
        assert np.array_equal(a[~fin], w[~fin], equal_nan=True), (what, k, a, w)
        err = np.abs(a[fin] - w[fin])
        assert bool((err <= rtol * np.abs(w[fin])).all()), (what, k, float((err / np.maximum(np.abs(w[fin]), 1e-300)).max()) if fin.any() else 0.0)


def call(name, spacing=None, device=None, dtypes=(torch.uint8, torch.uint8), **kw):
    case = SC.CASES[name]
    p, t = (torch.from_numpy(a != 0) if d == torch.bool else torch.from_numpy(a).to(d) for a, d in zip((case.pred, case.truth), dtypes))
    if device is not None:
        p, t = p.to(device), t.to(device)
    args = dict(background=case.background, dims=case.dims, connectivity=case.connectivity, percentile=case.percentile,
                tolerance=SC.TOLERANCES if spacing is None else SC.SPACING_TOLERANCES, spacing=None if spacing is None else spacing[-case.dims:])
    args.update(kw)
    return surface_metrics(p, t, case.labels, **args)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_host_form_against_the_yardstick(name):
    check(name, call(name), SC.expected(name), None, name)


@pytest.mark.parametrize("spacing", SC.SPACINGS, ids=str)
@pytest.mark.parametrize("name", SC.SPACING_CASES)
def test_host_form_with_spacing(name, spacing):
    check(name, call(name, spacing), SC.expected(name, spacing), spacing, (name, spacing))


@pytest.mark.parametrize("name", [n for n, c in SC.CASES.items() if c.pred.size <= SC.BRUTE_LIMIT])
def test_brute_force_equals_the_scipy_recipe(name):
    case = SC.CASES[name]
    conn = case.connectivity or (4 if case.dims == 2 else 6)
    for p, t in zip(SC._entries(case.pred, case.dims), SC._entries(case.truth, case.dims)):
        for op, ot in zip(SC.objects(p, case.labels, case.background), SC.objects(t, case.labels, case.background)):
            bp, bt = SC.surface(op, case.dims, conn), SC.surface(ot, case.dims, conn)
            for brute, recipe in zip(SC.brute_force(bp, bt), SC.sample_sets(bp, bt, None)):
                want = np.where(np.isfinite(recipe), np.rint(recipe * recipe), -1).astype(np.int64)
                assert np.array_equal(brute, want), name


def test_tolerances_with_spacing_are_clear_of_every_sample():
    for spacing in SC.SPACINGS:
        for name in SC.SPACING_CASES:
            d = SC.expected(name, spacing)["samples"]
            for tol in SC.SPACING_TOLERANCES:
                assert not (np.abs(d - tol) <= 1e-5 * tol).any(), (name, spacing, tol)


def test_empty_surface_conventions():
    blank, dot = torch.zeros((5, 6), dtype=torch.uint8), torch.zeros((5, 6), dtype=torch.uint8)
    dot[2, 3] = 1
    r = surface_metrics(blank, blank, tolerance=(0.0, 3.0))
    assert r["surface_count"].tolist() == [[0, 0]]
    for k in SC.KEYS1 + SC.KEYS2 + ("surface_dice",):
        assert bool(torch.isnan(r[k]).all()), k
    for a, b, empty in ((blank, dot, 0), (dot, blank, 1)):
        r = surface_metrics(a, b, tolerance=(0.0, 3.0, math.inf))
        assert r["surface_count"][0, empty] == 0 and r["surface_count"][0, 1 - empty] == 1
        for k in SC.KEYS2:
            assert math.isnan(r[k][0, empty]) and r[k][0, 1 - empty] == math.inf, k
        for k in SC.KEYS1:
            assert r[k][0] == math.inf, k
        assert r["surface_dice"].tolist() == [[0.0, 0.0, 0.0]]
    r = surface_metrics(dot, dot, percentile=0.0)                    # a weight of 0 takes the lower statistic as it is
    assert r["hausdorff_percentile"].item() == 0.0 and r["surface_dice"].item() == 1.0
    r = surface_metrics(torch.zeros((2, 0, 4), dtype=torch.int16), torch.zeros((2, 0, 4), dtype=torch.int64), (1, 2))
    assert r["surface_count"].shape == (2, 2, 2) and not r["surface_count"].any() and bool(torch.isnan(r["assd"]).all()) and r["assd"].shape == (2, 2)
    assert surface_metrics(torch.zeros((0, 3, 4), dtype=torch.uint8), torch.zeros((0, 3, 4), dtype=torch.uint8))["surface_dice"].shape == (0, 1, 1)


def test_validation_errors():
    a = torch.zeros((4, 5), dtype=torch.uint8)
    for bad, exc, match in (
            (dict(pred=a.numpy()), TypeError, "pred must be a tensor"),
            (dict(truth=a.float()), TypeError, "truth must hold integer labels"),
            (dict(pred=a.double()), TypeError, "pred must hold integer labels"),
            (dict(truth=torch.zeros((4, 6), dtype=torch.uint8)), ValueError, "same shape"),
            (dict(truth=a.to("meta")), ValueError, "same device"),
            (dict(dims=4), ValueError, "dims must be 2 or 3"),
            (dict(dims=3), ValueError, r"pred and truth must be \[\*stack, D, H, W\]"),
            (dict(connectivity=6), ValueError, "connectivity must be 4 or 8"),
            (dict(connectivity=True), ValueError, "connectivity must be 4 or 8"),
            (dict(labels=[]), ValueError, "at least one class"),
            (dict(labels=3), TypeError, "labels must be None or a sequence"),
            (dict(labels=[1.5]), TypeError, "labels must be an int"),
            (dict(background=None), TypeError, "background must be an int"),
            (dict(spacing=(1.0,)), ValueError, "spacing must have 2 entries"),
            (dict(spacing=(1.0, 0.0)), ValueError, "spacing must be positive"),
            (dict(spacing=2.0), TypeError, "spacing must be None or 2 floats"),
            (dict(percentile=101.0), ValueError, "percentile must lie in"),
            (dict(percentile=float("nan")), ValueError, "percentile must lie in"),
            (dict(percentile=(50.0, 95.0)), ValueError, "percentile must have 1 to 1"),
            (dict(percentile="high"), TypeError, "percentile must be a float"),
            (dict(tolerance=-1.0), ValueError, "tolerance must lie in"),
            (dict(tolerance=()), ValueError, "tolerance must have 1 to 8"),
            (dict(tolerance=(1.0,) * 9), ValueError, "tolerance must have 1 to 8"),
            (dict(tolerance=None), TypeError, "tolerance must be a float or a sequence"),
            (dict(max_workspace_bytes=0), ValueError, "max_workspace_bytes must be positive"),
            (dict(max_workspace_bytes=1.5), TypeError, "max_workspace_bytes must be an int")):
        kw = dict(pred=a, truth=a)
        kw.update(bad)
        pred, truth, labels = kw.pop("pred"), kw.pop("truth"), kw.pop("labels", None)
        with pytest.raises(exc, match=match):
            surface_metrics(pred, truth, labels, **kw)
    with pytest.raises(ValueError, match=r"connectivity must be 6 or 26"):
        surface_metrics(a[None], a[None], dims=3, connectivity=8)


def test_plan_refuses_what_it_cannot_serve():
    """host-only: the plan touches no device.  A stack whose two border maps pass the transform's position limit and a cap below the
    one-class minimum are raised, not ignored; the chunk is the largest that fits"""
    from pytorch_toolbelt_amd.utils import surface as S

    with pytest.raises(ValueError, match="split the stack"):
        S._workspace_plan((2, 30000, 30000), 1)
    plan = S._workspace_plan((3, 21, 45), 3)
    assert plan["chunk"] == 3 and plan["minimum"] < plan["bytes"]
    assert S._workspace_plan((3, 21, 45), 3, max_workspace_bytes=plan["minimum"])["chunk"] == 1
    assert S._workspace_plan((3, 21, 45), 3, max_workspace_bytes=plan["bytes"] - 1)["chunk"] == 2
    with pytest.raises(ValueError, match="is below the"):
        S._workspace_plan((3, 21, 45), 3, max_workspace_bytes=plan["minimum"] - 1)
    assert S._workspace_plan((5000, 5000), 100)["chunk"] < 32
    # the plan also answers for every launch's grid, so the call refuses nothing that the plan accepted.  Only the pick kernel's (three
    # workgroups per object) can pass 2^31 - 1 within the position limit: with more than 2^31 / 3 maps of a single position
    assert S._workspace_plan((1 << 29, 1, 1), 2, max_workspace_bytes=1 << 50)["chunk"] == 1
    with pytest.raises(ValueError, match="split the stack"):
        S._workspace_plan(((1 << 30) - 1, 1, 1), 1, max_workspace_bytes=1 << 50)
    for bad, exc, match in (((dict(classes=0)), ValueError, "classes must be positive"), (dict(classes=2.5), TypeError, "classes must be an int"),
                            (dict(max_workspace_bytes=1.5), TypeError, "max_workspace_bytes must be an int"), (dict(dims=4), ValueError, "dims must be 2 or 3"),
                            (dict(shape=(4,)), ValueError, "pred and truth must be")):
        kw = dict(shape=(4, 5))
        kw.update(bad)
        with pytest.raises(exc, match=match):
            S._workspace_plan(**kw)
