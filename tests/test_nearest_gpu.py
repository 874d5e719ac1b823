"""GPU: the feature-transform kernels (csrc/ptb_nearest.hip) against the restatements of tests/nearest_cases.py.

  index, unit spacing        equal to the brute force (smallest linear index on a tie) on every case of at most BRUTE_LIMIT positions per
                             entry; on the four larger ones a site at scipy's exact distance; on all 111 equal to the host form.
  spacing, powers of two     equal to the weighted brute force: every value a pass stores is exact in float32 (asserted by the cases).
  spacing (2.5, 0.7, 0.7)    validity: the float64 distance to the returned site is at most the float64 minimum times (1 + 1e-6), the
  and (1, 1, 3)              bound tests/test_distance_gpu.py holds the spacing form of the distance itself to.
  return_distance            the bits of ``distance_transform(squared=True)`` on the device.
  expand_labels              equal to the definition, position by position, on every expansion case."""
import numpy as np
import pytest
import torch

import distance_cases as DC
import nearest_cases as NC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import connected_components, distance_transform, expand_labels, match_instances, nearest_site

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = (torch.bool, torch.int16, torch.int32, torch.int64)
NP = {torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64}
DTYPE_CASES = ("blobs", "noise_2T+1", "stack_hole", "len257_x", "len65_y", "sparse_W%4", "volume_blobs", "volume_stack_hole", "len129_z3") + DC.OFFSET_CASES


def _offset(t):
    """a contiguous device copy of ``t`` that starts one element into its buffer: the peeled loads"""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def _dev(name, dtype=torch.uint8):
    a, dims = NC.CASES[name]
    t = torch.from_numpy((a != 0) if dtype == torch.bool else a.astype(NP[dtype]))
    return (_offset(t) if name in DC.OFFSET_CASES else t.to(DEV)), dims


def _near(t, **kw):
    before = N.calls
    res = nearest_site(t, **kw)
    assert N.calls == before + 1, "one native call per transform"
    index = res[0] if kw.get("return_distance") else res
    assert index.dtype == torch.int32 and index.shape == t.shape and index.device == DEV
    return res


def _expand(case, **kw):
    m = torch.from_numpy(case.markers)
    m = _offset(m) if case.offset else m.to(DEV)
    mask = None if case.mask is None else torch.from_numpy(case.mask).to(DEV)
    args = dict(distance=case.distance, mask=mask, background=case.background, dims=case.dims, spacing=case.spacing)
    args.update(kw)
    before = N.calls
    got = expand_labels(m, **args)
    assert N.calls == before + 1 and got.dtype == m.dtype and got.shape == m.shape and got.device == DEV
    return got, m


@pytest.mark.parametrize("name", list(NC.CASES))
def test_index_against_the_restatement_and_the_host_form(name):
    t, dims = _dev(name)
    got = _near(t, dims=dims).cpu()
    if name in NC.SMALL:
        assert np.array_equal(got.numpy(), NC.expected_index(name)), name
    else:
        NC.check_valid(got.numpy(), name)
    assert torch.equal(got, nearest_site(torch.from_numpy(NC.CASES[name][0]), dims=dims)), (name, "host form")


@pytest.mark.parametrize("name", DTYPE_CASES)
def test_every_element_type_in_both_load_arms(name):
    t, dims = _dev(name)
    want = _near(t, dims=dims)
    for dtype in DTYPES:
        t, dims = _dev(name, dtype)
        assert torch.equal(_near(t, dims=dims), want), (name, dtype)


@pytest.mark.parametrize("name", DC.OFFSET_CASES)
def test_misaligned_base(name):
    t, dims = _dev(name)
    assert t.data_ptr() % 16 != 0
    aligned = torch.from_numpy(NC.CASES[name][0]).to(DEV)
    assert torch.equal(_near(t, dims=dims), _near(aligned, dims=dims)), name


@pytest.mark.parametrize("spacing", NC.EXACT_SPACINGS, ids=str)
@pytest.mark.parametrize("name", NC.EXACT_SPACING_CASES)
def test_exact_spacing_against_the_weighted_brute_force(name, spacing):
    t, dims = _dev(name)
    got = _near(t, dims=dims, spacing=spacing[-dims:]).cpu()
    assert np.array_equal(got.numpy(), NC.expected_index_spacing(name, spacing)), (name, spacing)
    assert torch.equal(got, nearest_site(torch.from_numpy(NC.CASES[name][0]), dims=dims, spacing=spacing[-dims:])), (name, spacing, "host form")


@pytest.mark.parametrize("spacing", DC.SPACINGS, ids=str)
@pytest.mark.parametrize("name", DC.SPACING_CASES)
def test_spacing_names_a_nearest_site(name, spacing):
    t, dims = _dev(name)
    a = NC.CASES[name][0]
    got = _near(t, dims=dims, spacing=spacing[-dims:]).cpu().numpy().astype(np.int64)
    want = DC.expected_spacing(name, spacing)
    none = ~np.isfinite(want)
    assert np.array_equal(got < 0, none) and bool((got[none] == -1).all()), (name, spacing)
    entries = len(DC._entries(a, dims))
    named = np.take_along_axis((a == 0).reshape(entries, -1), np.maximum(got, 0).reshape(entries, -1), axis=1).reshape(a.shape)
    assert bool(named[~none].all()), (name, spacing, "not a site")
    d = NC.squared_to(np.maximum(got, 0), a.shape, dims, spacing)
    worst = float((d[~none] / np.maximum(want[~none], 1e-300))[want[~none] > 0].max()) if (want[~none] > 0).any() else 1.0
    print(f"{name} {spacing}: worst squared-distance ratio {worst:.9f}")
    assert bool((np.sqrt(d[~none]) <= np.sqrt(want[~none]) * (1 + 1e-6)).all()), (name, spacing, worst)


@pytest.mark.parametrize("name", ("blobs", "stack_hole", "sparse_offset", "volume_stack_hole", "len257_z3", "wide_one_site", "volume_big"))
def test_return_distance_has_the_bits_of_distance_transform(name):
    t, dims = _dev(name)
    for kw in (dict(), dict(spacing=DC.SPACINGS[0][-dims:]), dict(spacing=NC.EXACT_SPACINGS[1][-dims:]), dict(foreground=1)):
        index, sq = _near(t, dims=dims, return_distance=True, **kw)
        want = distance_transform(t, dims=dims, squared=True, **kw)
        assert sq.dtype == want.dtype and torch.equal(sq.view(torch.int32), want.view(torch.int32)), (name, kw)
        assert torch.equal(index, _near(t, dims=dims, **kw)), (name, kw)


def test_out_receives_the_index():
    for name in ("blobs", "volume_blobs"):
        t, dims = _dev(name)
        want = _near(t, dims=dims)
        out = torch.full(t.shape, 7, dtype=torch.int32, device=DEV)
        assert _near(t, dims=dims, out=out) is out and torch.equal(out, want)
        index, sq = _near(t, dims=dims, out=out.fill_(7), return_distance=True)
        assert index is out and torch.equal(out, want) and torch.equal(sq, distance_transform(t, dims=dims, squared=True))
        view = _offset(torch.zeros(t.shape, dtype=torch.int32))                # an out that is not 16-byte aligned still receives it
        assert _near(t, dims=dims, out=view) is view and torch.equal(view, want)
    with pytest.raises(ValueError, match="out must be"):
        nearest_site(t, dims=dims, out=torch.zeros(t.shape, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match="mask must have shape"):
        expand_labels(t, dims=dims, mask=torch.ones(t.shape, dtype=torch.bool))       # a mask on another device


@pytest.mark.parametrize("case", NC.EXPANSIONS, ids=repr)
def test_expansion_equals_the_definition(case):
    got, m = _expand(case)
    assert np.array_equal(got.cpu().numpy(), case.expected), case
    assert torch.equal(_expand(case, distance=0)[0], m), "distance=0 returns the markers"
    out = torch.zeros_like(got)
    assert _expand(case, out=out)[0] is out and torch.equal(out, got)


def test_expansion_out_may_be_the_markers_or_misaligned():
    case = next(c for c in NC.EXPANSIONS if c.distance == 2.5 and c.mask is None)
    got, m = _expand(case)
    view = _offset(torch.zeros(m.shape, dtype=m.dtype))
    assert expand_labels(m, distance=case.distance, dims=case.dims, out=view) is view and torch.equal(view, got)
    work = m.clone()
    assert expand_labels(work, distance=case.distance, dims=case.dims, out=work) is work and torch.equal(work, got)


def test_two_disc_split_on_the_device():
    sem, truth = NC.two_discs()
    t = torch.from_numpy(sem).to(DEV)
    assert int(connected_components(t)[1]) == 1
    cores, n = connected_components(distance_transform(t) > 8)
    assert int(n) == 2 and int(n) >= 0
    inst = expand_labels(cores, mask=t != 0)
    assert inst.dtype == torch.int32 and int((inst != 0).sum()) == 573 and sorted(np.unique(inst.cpu().numpy())) == [0, 1, 2]
    res = match_instances(inst, torch.from_numpy(truth).to(DEV), thresholds=(0.5,), num_pred=2, num_truth=2)
    assert int(res["tp"][0]) == 2 and int(res["fp"][0]) == 0 and int(res["fn"][0]) == 0
    assert bool((res["pred_iou"] >= 0.9).all()), res["pred_iou"]
    assert torch.equal(inst.cpu(), expand_labels(cores.cpu(), mask=torch.from_numpy(sem != 0)))


@pytest.mark.parametrize("name", DC.BIG_CASES)
def test_two_runs_are_bit_identical(name):
    t, dims = _dev(name)
    for kw in (dict(), dict(spacing=DC.SPACINGS[0][-dims:])):
        a, b = _near(t, dims=dims, return_distance=True, **kw), _near(t, dims=dims, return_distance=True, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), (name, kw)
    cores = (distance_transform(t, dims=dims, squared=True) > 8).to(torch.int32) * 3
    assert torch.equal(expand_labels(cores, distance=20.0, dims=dims, mask=t != 0), expand_labels(cores, distance=20.0, dims=dims, mask=t != 0)), name


def test_non_default_stream_and_non_contiguous_input():
    a, dims = NC.CASES["blobs"]
    t = torch.from_numpy(a).to(DEV)
    markers = torch.from_numpy(NC.sparse_markers(a.shape, 360)).to(DEV)
    want, want_e = _near(t), expand_labels(markers, distance=9.0, mask=t != 0)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        got, got_e = _near(t), expand_labels(markers, distance=9.0, mask=t != 0)
    torch.cuda.current_stream(DEV).wait_stream(stream)
    assert torch.equal(got, want) and torch.equal(got_e, want_e)
    wide = torch.from_numpy(np.ascontiguousarray(a.T)).to(DEV).t()                       # the same map with other strides
    assert not wide.is_contiguous() and torch.equal(_near(wide), want)
    every_other = torch.from_numpy(np.repeat(a, 2, axis=1)).to(DEV)[:, ::2]
    assert not every_other.is_contiguous() and torch.equal(_near(every_other), want)
    m2 = torch.repeat_interleave(markers, 2, dim=1)[:, ::2]
    k2 = torch.repeat_interleave(t != 0, 2, dim=1)[:, ::2]
    assert not m2.is_contiguous() and torch.equal(expand_labels(m2, distance=9.0, mask=k2), want_e)


def test_empty_inputs_launch_nothing():
    before = N.calls
    d = nearest_site(torch.zeros((0, 5), dtype=torch.uint8, device=DEV))
    assert d.shape == (0, 5) and d.dtype == torch.int32 and d.device == DEV
    index, sq = nearest_site(torch.zeros((2, 3, 0), dtype=torch.int64, device=DEV), dims=3, return_distance=True)
    assert index.shape == sq.shape == (2, 3, 0) and sq.dtype == torch.int32 and sq.device == DEV
    e = expand_labels(torch.zeros((0, 4, 5), dtype=torch.int16, device=DEV), distance=1.0)
    assert e.shape == (0, 4, 5) and e.dtype == torch.int16 and e.device == DEV
    assert N.calls == before
