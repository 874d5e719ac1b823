"""GPU: the surface-metric kernels (csrc/ptb_surface.hip) against the scipy yardstick of tests/surface_cases.py.

  surface_count, surface Dice      equal integers: surface Dice must be float32(within / total) of the yardstick's counts, bit for bit
  Hausdorff, unit spacing          float32(sqrt(float64(exact squared integer))), bit for bit
  percentiles, means, assd         unit spacing: rtol 1e-6 -- one float32 rounding (6e-8) of a value computed in double from exact integers,
                                   plus the yardstick's own float64 transform
  everything with ``spacing``      rtol 2e-6: the transform is held to 1e-6 against scipy in test_distance_gpu.py; maximum, interpolation and
                                   mean of non-negative values keep that bound; then one more rounding
``inf`` / ``nan`` exactly where the yardstick has them."""
import numpy as np
import pytest
import torch

import surface_cases as SC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import surface as S
from pytorch_toolbelt_amd.utils import surface_metrics
from test_surface_cpu import check

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
INTS = (torch.uint8, torch.int16, torch.int32, torch.int64)


def _dev(a, dtype, offset):
    t = torch.from_numpy(a != 0) if dtype == torch.bool else torch.from_numpy(a).to(dtype)
    if not offset:
        return t.to(DEV)
    buf = torch.zeros(t.numel() + 1, dtype=dtype, device=DEV)       # a contiguous view that starts one element into its buffer: the peeled loads
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and (dtype == torch.int64 or view.data_ptr() % 16 != 0)
    return view


def run(name, spacing=None, dtypes=(torch.uint8, torch.uint8), **kw):
    case = SC.CASES[name]
    p, t = (_dev(a, d, name in SC.OFFSET_CASES) for a, d in zip((case.pred, case.truth), dtypes))
    args = dict(background=case.background, dims=case.dims, connectivity=case.connectivity, percentile=case.percentile,
                tolerance=SC.TOLERANCES if spacing is None else SC.SPACING_TOLERANCES, spacing=None if spacing is None else spacing[-case.dims:])
    args.update(kw)
    before = N.calls
    res = surface_metrics(p, t, case.labels, **args)
    assert N.calls == before + 1, "one native metrics call per public call"
    assert all(v.device == DEV for v in res.values())
    return res


def same_bits(a, b):
    return set(a) == set(b) and all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                                b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]) for k in a)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_against_the_yardstick(name):
    check(name, run(name), SC.expected(name), None, name)


@pytest.mark.parametrize("spacing", SC.SPACINGS, ids=str)
@pytest.mark.parametrize("name", SC.SPACING_CASES)
def test_with_spacing_against_the_yardstick(name, spacing):
    check(name, run(name, spacing), SC.expected(name, spacing), spacing, (name, spacing))


@pytest.mark.parametrize("name", SC.DTYPE_CASES)
def test_every_dtype_and_mixed_dtypes(name):
    want = run(name)
    for dp in INTS:
        for dt in INTS:
            assert same_bits(run(name, dtypes=(dp, dt)), want), (name, dp, dt)
    check(name, want, SC.expected(name), None, name)


def test_bool_maps():
    want = run("stack_objects")
    for dp, dt in ((torch.bool, torch.bool), (torch.bool, torch.int32), (torch.int64, torch.bool)):
        assert same_bits(run("stack_objects", dtypes=(dp, dt)), want), (dp, dt)
    check("stack_objects", want, SC.expected("stack_objects"), None, "bool")


@pytest.mark.parametrize("name", SC.BIG_CASES)
def test_two_runs_are_bit_identical(name):
    for spacing in (None, SC.SPACINGS[0]):
        assert same_bits(run(name, spacing), run(name, spacing)), (name, spacing)


@pytest.mark.parametrize("name", ("stack", "volume_stack"))
def test_chunking_changes_no_bit(name):
    """K = 3 in one chunk (the default) against one class at a time (the least cap accepted) and against 2 + 1 (a partial last chunk)"""
    case = SC.CASES[name]
    plan = S._workspace_plan(case.pred.shape, len(case.labels), case.dims)
    assert plan["chunk"] == len(case.labels) == 3
    least = S._workspace_plan(case.pred.shape, len(case.labels), case.dims, max_workspace_bytes=plan["minimum"])
    assert least["chunk"] == 1 and least["bytes"] == plan["minimum"]
    assert S._workspace_plan(case.pred.shape, len(case.labels), case.dims, max_workspace_bytes=plan["bytes"] - 1)["chunk"] == 2
    for spacing in (None, SC.SPACINGS[0]):
        want = run(name, spacing)
        assert same_bits(run(name, spacing, max_workspace_bytes=plan["minimum"]), want), (name, spacing, "1 + 1 + 1")
        assert same_bits(run(name, spacing, max_workspace_bytes=plan["bytes"] - 1), want), (name, spacing, "2 + 1")
    with pytest.raises(ValueError, match="is below the"):
        run(name, max_workspace_bytes=plan["minimum"] - 1)


def test_more_classes_than_a_chunk_takes():
    """K = 40 at the default cap is 32 + 8; a cap for about 7 classes gives several full chunks and a partial one (7 x 5 + 5): the same
    bits, and those of the classes scored in two calls of 20"""
    name = "many_classes"
    case = SC.CASES[name]
    K = len(case.labels)
    plan = S._workspace_plan(case.pred.shape, K, case.dims)
    assert K == 40 and plan["chunk"] == 32
    cap = plan["minimum"] + 13 * (plan["bytes"] - plan["minimum"]) // 62        # the bytes of 32 classes less those of 1, over 31: a class; 6.5 of them
    some = S._workspace_plan(case.pred.shape, K, case.dims, max_workspace_bytes=cap)["chunk"]
    assert 1 < some < 32 and K % some, some
    for spacing in (None, SC.SPACINGS[0]):
        want = run(name, spacing)
        check(name, want, SC.expected(name, spacing), spacing, (name, spacing))
        assert same_bits(run(name, spacing, max_workspace_bytes=cap), want), (spacing, some)
        p, t = (torch.from_numpy(a).to(DEV) for a in (case.pred, case.truth))
        kw = dict(tolerance=SC.TOLERANCES if spacing is None else SC.SPACING_TOLERANCES, spacing=None if spacing is None else spacing[-2:])
        halves = [surface_metrics(p, t, case.labels[i:i + 20], **kw) for i in (0, 20)]
        assert same_bits({k: torch.cat([h[k] for h in halves], dim=1) for k in want}, want), (spacing, "20 | 20")


@pytest.mark.parametrize("name", ("stack", "long_thin", "volume_blobs_c26", "squares_p95"))
def test_device_equals_the_host_form(name):
    """within the bounds of the yardstick tests (rtol 1e-6 with unit spacing, 2e-6 with spacing); counts, surface Dice and the unit-spacing
    maxima bit for bit"""
    case = SC.CASES[name]
    for spacing in (None, SC.SPACINGS[1]):
        got = {k: v.cpu() for k, v in run(name, spacing).items()}
        kw = dict(background=case.background, dims=case.dims, connectivity=case.connectivity, percentile=case.percentile,
                  tolerance=SC.TOLERANCES if spacing is None else SC.SPACING_TOLERANCES, spacing=None if spacing is None else spacing[-case.dims:])
        host = surface_metrics(torch.from_numpy(case.pred), torch.from_numpy(case.truth), case.labels, **kw)
        assert torch.equal(got["surface_count"], host["surface_count"])
        assert torch.equal(got["surface_dice"].view(torch.int32), host["surface_dice"].view(torch.int32))
        if spacing is None:
            assert torch.equal(got["directed_hausdorff"].view(torch.int32), host["directed_hausdorff"].view(torch.int32))
            assert torch.equal(got["hausdorff"].view(torch.int32), host["hausdorff"].view(torch.int32))
        for k in SC.KEYS1 + SC.KEYS2:
            a, w = got[k].double().numpy(), host[k].double().numpy()
            fin = np.isfinite(w)
            assert np.array_equal(a[~fin], w[~fin], equal_nan=True), (name, k)
            err = np.abs(a[fin] - w[fin])
            assert bool((err <= (1e-6 if spacing is None else 2e-6) * np.abs(w[fin])).all()), (name, k, spacing, float(err.max()) if fin.any() else 0.0)


def test_other_strides_and_streams():
    case = SC.CASES["blobs_c8"]
    want = run("blobs_c8")
    p = torch.from_numpy(np.ascontiguousarray(case.pred.T)).to(DEV).t()
    t = torch.from_numpy(np.repeat(case.truth, 2, axis=1)).to(DEV)[:, ::2]
    assert not p.is_contiguous() and not t.is_contiguous()
    kw = dict(connectivity=8, tolerance=SC.TOLERANCES)
    assert same_bits(surface_metrics(p, t, case.labels, **kw), want)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        got = surface_metrics(p, t, case.labels, **kw)
    torch.cuda.current_stream(DEV).wait_stream(stream)
    assert same_bits(got, want)


def test_inputs_out_of_contract_raise_before_a_launch():
    a = torch.zeros((4, 5), dtype=torch.uint8, device=DEV)
    before = N.calls
    with pytest.raises(ValueError, match="same shape"):
        surface_metrics(a, a[:, :4])
    with pytest.raises(ValueError, match="same device"):
        surface_metrics(a, a.cpu())
    with pytest.raises(TypeError, match="must hold integer labels"):
        surface_metrics(a.float(), a)
    with pytest.raises(TypeError, match="must hold integer labels"):
        surface_metrics(a, a.half())
    empty = surface_metrics(a[:0], a[:0], (1, 2))
    assert empty["surface_count"].shape == (2, 2) and empty["surface_count"].device == DEV
    assert N.calls == before
