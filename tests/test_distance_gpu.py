"""GPU: the distance-transform kernels (csrc/ptb_distance.hip) against the exact squared distances of tests/distance_cases.py.

  squared=True, unit spacing (int32)   equal to the expected integers bit for bit, on every case, every input dtype, both ``dims``.
  default float32, unit spacing        rtol 5e-7, atol 0 against sqrt of the exact integers in float64: the int -> float32 conversion is at
                                       most 1/2 ulp (exact below 2^24), sqrtf at most 1 ulp, and an ulp is 2^-23 = 1.2e-7 relative.
  spacing (2.5, 0.7, 0.7) / (1, 1, 3)  rtol 1e-6, atol 0 against scipy's ``sampling=`` in float64: one float32 rounding per pass and the root.
  signed=True                          int32 form equal bit for bit to expected(object) - expected(sites); float forms with the bounds above.
``inf`` positions must be ``inf`` exactly."""
import numpy as np
import pytest
import torch

import distance_cases as DC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import distance_transform, remove_small_components

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = (torch.bool, torch.uint8, torch.int16, torch.int32, torch.int64)
NP = {torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64}


def _dev(name, dtype=torch.uint8):
    a, dims = DC.CASES[name]
    t = torch.from_numpy((a != 0) if dtype == torch.bool else a.astype(NP[dtype]))
    if name in DC.OFFSET_CASES:                      # a contiguous view that starts one element into its buffer: the peeled loads
        buf = torch.zeros(t.numel() + 1, dtype=dtype, device=DEV)
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        return view, dims
    return t.to(DEV), dims


def _edt(t, **kw):
    before = N.calls
    d = distance_transform(t, **kw)
    assert N.calls == before + 1, "one native call per transform"
    want = torch.int32 if kw.get("squared") and kw.get("spacing") is None else torch.float32
    assert d.dtype == want and d.shape == t.shape and d.device == DEV
    return d


def _close(got, want, rtol, what):
    """got (float32 tensor) against want (float64 array): inf where want is inf (with its sign), rtol elsewhere, atol 0"""
    got = got.cpu().numpy().astype(np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), what
    err = np.abs(got[fin] - want[fin])
    bound = rtol * np.abs(want[fin])
    worst = float((err / np.maximum(np.abs(want[fin]), 1e-300)).max()) if fin.any() else 0.0
    assert bool((err <= bound).all()), (what, f"worst relative error {worst:.3e} > {rtol}")


@pytest.mark.parametrize("name", list(DC.CASES))
def test_squared_int32_is_exact_for_every_dtype(name):
    want = DC.expected(name)
    for dtype in DTYPES:
        t, dims = _dev(name, dtype)
        got = _edt(t, dims=dims, squared=True)
        assert np.array_equal(got.cpu().numpy(), want), (name, dtype)


@pytest.mark.parametrize("name", list(DC.CASES))
def test_float32_distances(name):
    t, dims = _dev(name)
    _close(_edt(t, dims=dims), DC.as_float(DC.expected(name)), 5e-7, name)


@pytest.mark.parametrize("spacing", DC.SPACINGS, ids=str)
@pytest.mark.parametrize("name", DC.SPACING_CASES)
def test_spacing_against_scipy(name, spacing):
    t, dims = _dev(name)
    sq = DC.expected_spacing(name, spacing)
    _close(_edt(t, dims=dims, spacing=spacing[-dims:]), np.sqrt(sq), 1e-6, (name, spacing))
    _close(_edt(t, dims=dims, spacing=spacing[-dims:], squared=True), sq, 1e-6, (name, spacing, "squared"))


@pytest.mark.parametrize("name", DC.SIGNED_CASES)
def test_signed(name):
    t, dims = _dev(name)
    want = DC.expected_signed(name)
    got = _edt(t, dims=dims, squared=True, signed=True)
    assert np.array_equal(got.cpu().numpy(), want), name
    _close(_edt(t, dims=dims, signed=True), DC.as_float(DC.expected(name, True)) - DC.as_float(DC.expected(name)), 5e-7, name)
    if name in DC.SPACING_CASES:
        sp = DC.SPACINGS[0]
        _close(_edt(t, dims=dims, signed=True, spacing=sp[-dims:]), np.sqrt(DC.expected_spacing(name, sp, True)) - np.sqrt(DC.expected_spacing(name, sp)), 1e-6, name)


def test_signed_entries_that_are_all_object_or_all_sites():
    for name, sign in (("ones", -1), ("volume_ones", -1), ("zeros", 1)):
        t, dims = _dev(name)
        assert bool((_edt(t, dims=dims, squared=True, signed=True) == sign * DC.INF).all()), name
        assert bool((_edt(t, dims=dims, signed=True) == sign * float("inf")).all()), name
        assert bool((_edt(t, dims=dims, signed=True, spacing=(2.0,) * dims) == sign * float("inf")).all()), name
    hole, dims = _dev("stack_hole")
    got = _edt(hole, dims=dims, signed=True)
    assert bool((got[1] == -float("inf")).all()) and bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[2]).all())


@pytest.mark.parametrize("name", DC.FOREGROUND_CASES + ("volume_blobs",))
def test_foreground_class_equals_the_boolean_map(name):
    a, dims = DC.CASES[name]
    t = torch.from_numpy(a).to(DEV)
    for c in list(range(int(a.max()) + 2)) + [300, -1]:          # one class that does not occur; values uint8 cannot hold
        mask = torch.from_numpy(a.astype(np.int64) == c).to(DEV)
        want = _edt(mask, dims=dims, squared=True)               # sites of a bool map: its zeros
        got = _edt(t, foreground=c, dims=dims, squared=True)
        assert torch.equal(got, want), (name, c)
        if name in DC.FOREGROUND_CASES:
            assert np.array_equal(got.cpu().numpy(), DC.brute_force(a != c, dims)), (name, c)
        if c > int(a.max()):
            assert not got.any(), "a class that occurs nowhere: every position is a site"
    wide = torch.from_numpy(a.astype(np.int64)).to(DEV)
    assert torch.equal(_edt(wide, foreground=2, dims=dims, squared=True), _edt(t, foreground=2, dims=dims, squared=True))
    assert bool((_edt(t, background=300, dims=dims, squared=True) == DC.INF).all()), "a background that occurs nowhere: no site"
    other = _edt(t, background=1, dims=dims, squared=True)
    assert np.array_equal(other.cpu().numpy(), DC.restate(a == 1, dims)), name


def test_out_receives_the_result():
    t, dims = _dev("blobs")
    for kw, dtype in ((dict(squared=True), torch.int32), (dict(), torch.float32), (dict(signed=True, spacing=(0.5, 2.0)), torch.float32)):
        want = _edt(t, **kw)
        out = torch.full(t.shape, 7, dtype=dtype, device=DEV)
        assert _edt(t, out=out, **kw) is out and torch.equal(out, want)
        buf = torch.zeros(t.numel() + 1, dtype=dtype, device=DEV)          # an out that is not 16-byte aligned still receives it
        view = buf[1:].view(t.shape)
        assert _edt(t, out=view, **kw) is view and torch.equal(view, want)
    with pytest.raises(ValueError, match="out must be"):
        distance_transform(t, out=torch.zeros(t.shape, dtype=torch.int32, device=DEV))


def test_non_default_stream_and_non_contiguous_input():
    a, dims = DC.CASES["blobs"]
    t = torch.from_numpy(a).to(DEV)
    want, want_signed = _edt(t, squared=True), _edt(t, signed=True)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        got, got_signed = _edt(t, squared=True), _edt(t, signed=True)
    torch.cuda.current_stream(DEV).wait_stream(stream)
    assert torch.equal(got, want) and torch.equal(got_signed, want_signed)
    wide = torch.from_numpy(np.ascontiguousarray(a.T)).to(DEV).t()                       # the same map with other strides
    assert not wide.is_contiguous() and torch.equal(_edt(wide, squared=True), want)
    every_other = torch.from_numpy(np.repeat(a, 2, axis=1)).to(DEV)[:, ::2]
    assert not every_other.is_contiguous() and torch.equal(_edt(every_other, squared=True), want)


@pytest.mark.parametrize("name", DC.BIG_CASES)
def test_two_runs_are_bit_identical(name):
    t, dims = _dev(name)
    for kw in (dict(squared=True), dict(signed=True), dict(spacing=DC.SPACINGS[0][-dims:])):
        assert torch.equal(_edt(t, dims=dims, **kw), _edt(t, dims=dims, **kw)), (name, kw)


def test_empty_inputs_launch_nothing():
    before = N.calls
    d = distance_transform(torch.zeros((0, 5), dtype=torch.uint8, device=DEV))
    assert d.shape == (0, 5) and d.dtype == torch.float32 and d.device == DEV
    d = distance_transform(torch.zeros((0, 4, 5), dtype=torch.int64, device=DEV), squared=True)
    assert d.shape == (0, 4, 5) and d.dtype == torch.int32
    assert distance_transform(torch.zeros((2, 3, 0), dtype=torch.bool, device=DEV), dims=3, signed=True).shape == (2, 3, 0)
    assert N.calls == before


def test_interior_distance_of_the_cleaned_map():
    """the pipeline: merge_crop(argmax) -> remove_small_components -> interior distance, against the host route on the same map"""
    from scipy.ndimage import distance_transform_edt

    a, dims = DC.CASES["blobs_wide"]
    clean = remove_small_components(torch.from_numpy(a).to(DEV), min_area=30, connectivity=8)
    got = _edt(clean)
    host = distance_transform_edt(clean.cpu().numpy() != 0)
    assert (clean == 0).any()
    _close(got, host, 5e-7, "pipeline")
    assert np.array_equal(_edt(clean, squared=True).cpu().numpy(), np.rint(host * host).astype(np.int64))
