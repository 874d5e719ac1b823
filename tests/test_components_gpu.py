"""GPU: the connected-component kernels (csrc/ptb_components.hip) equal the flood fill of tests/components_cases.py exactly -- component
numbers, counts, areas and boxes are integers -- over the whole case list, every dtype and both connectivities of each ``dims``.  Every
count is asserted >= 0: -1 would mean that a lane ran into a step cap of the union-find.  All inputs are valid maps."""
import numpy as np
import pytest
import torch

import components_cases as C
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import component_stats, connected_components, remove_small_components, rle_encode_device

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = (torch.bool, torch.uint8, torch.int16, torch.int32, torch.int64)
NP = {torch.uint8: np.uint8, torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64}


def _host(name, dtype):
    a, dims = C.CASES[name]
    return (a != 0) if dtype == torch.bool else a.astype(NP[dtype]), dims


def _dev(name, dtype):
    a, dims = _host(name, dtype)
    t = torch.from_numpy(a)
    if name in C.OFFSET_CASES:                       # a contiguous view that starts one element into its buffer: the peeled loads
        buf = torch.zeros(t.numel() + 1, dtype=dtype, device=DEV)
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        return view, dims
    return t.to(DEV), dims


def _label(t, **kw):
    before = N.calls
    cc, count = connected_components(t, **kw)
    assert N.calls == before + 1, "one native call per labelling"
    assert cc.dtype == torch.int32 and cc.shape == t.shape and cc.device == DEV
    assert count.dtype == torch.int64 and count.device == DEV
    assert bool((count >= 0).all()), f"a step cap was exceeded: count = {count.tolist()}"
    return cc, count


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("name", list(C.CASES))
def test_labelling_equals_the_flood_fill(name, dtype):
    t, dims = _dev(name, dtype)
    for conn in C.CONNECTIVITIES[dims]:
        want = C.expected(name, conn, as_bool=dtype == torch.bool)
        cc, count = _label(t, connectivity=conn, dims=dims)
        assert count.shape == want["count"].shape
        assert np.array_equal(count.cpu().numpy(), want["count"]), (name, conn, count.tolist(), want["count"].tolist())
        assert np.array_equal(cc.cpu().numpy(), want["cc"]), (name, conn)


@pytest.mark.parametrize("name", ["blobs", "noise4_wide", "touching", "volume_blobs"])
def test_background_none_and_other_backgrounds(name):
    a, dims = C.CASES[name]
    t = torch.from_numpy(a).to(DEV)
    for conn in C.CONNECTIVITIES[dims]:
        for bg in (None, 1, 300):                    # 300: uint8 cannot hold it, so it occurs nowhere
            want = C.restate(a, dims, conn, background=bg)
            cc, count = _label(t, connectivity=conn, background=bg, dims=dims)
            assert np.array_equal(cc.cpu().numpy(), want["cc"]) and int(count) == int(want["count"]), (name, conn, bg)


@pytest.mark.parametrize("name", ["blobs", "noise4_wide", "ones", "speckle", "serpentine", "volume_blobs", "volume_noise_2T+1", "volume_ones"])
def test_component_stats_are_exact(name):
    a, dims = C.CASES[name]
    t = torch.from_numpy(a).to(DEV)
    for conn in C.CONNECTIVITIES[dims]:
        want = C.expected(name, conn)
        n = int(want["count"])
        cc, count = _label(t, connectivity=conn, dims=dims)
        before = N.calls
        got = component_stats(cc, count, values=t)
        assert N.calls == before + 1
        assert got["area"].dtype == torch.int64 and got["bbox"].dtype == torch.int64 and got["value"].dtype == t.dtype
        assert np.array_equal(got["area"].cpu().numpy(), want["areas"][0]), (name, conn)
        assert np.array_equal(got["bbox"].cpu().numpy(), want["boxes"][0]), (name, conn)
        assert np.array_equal(got["value"].cpu().numpy(), want["values"][0]), (name, conn)
        assert torch.equal(component_stats(cc)["area"], got["area"])                     # n from cc.max(), no values
        more = component_stats(cc, values=t, max_components=n + 3)                       # no read-back: rows past the count are empty
        assert torch.equal(more["area"][:n], got["area"]) and torch.equal(more["bbox"][:n], got["bbox"]) and torch.equal(more["value"][:n], got["value"])
        assert not more["area"][n:].any() and not more["bbox"][n:].any() and not more["value"][n:].any()
        if n > 1:                                                                        # components numbered above it are left out
            fewer = component_stats(cc, values=t, max_components=n - 1)
            assert torch.equal(fewer["area"], got["area"][:n - 1]) and torch.equal(fewer["bbox"], got["bbox"][:n - 1])


def test_component_stats_refuses_a_stack():
    t = torch.from_numpy(C.CASES["stack"][0]).to(DEV)
    cc, count = _label(t)
    with pytest.raises(ValueError, match="loop"):
        component_stats(cc, count)
    got = component_stats(cc[1], count[1])
    assert np.array_equal(got["area"].cpu().numpy(), C.expected("stack", 8)["areas"][1])


@pytest.mark.parametrize("name", ["blobs", "noise4_wide", "noise_offset", "speckle", "stack", "ones", "volume_blobs", "volume_stack"])
def test_remove_small_equals_the_flood_fill(name):
    a, dims = C.CASES[name]
    for conn in C.CONNECTIVITIES[dims]:
        ref = C.expected(name, conn)
        largest = max(int(x.max()) if x.size else 0 for x in ref["areas"])
        for min_area in (1, 2, 5, largest + 1):
            want = C.remove_small(a, dims, conn, min_area, ref=ref)
            t, _ = _dev(name, torch.uint8)
            before = N.calls
            got = remove_small_components(t, min_area, connectivity=conn, dims=dims)
            assert N.calls == before + 1 and got.dtype == t.dtype and got is not t
            assert np.array_equal(got.cpu().numpy(), want), (name, conn, min_area)
            assert np.array_equal(t.cpu().numpy(), a), "the input was written to"
            same = remove_small_components(t, min_area, connectivity=conn, dims=dims, out=t)     # in place
            assert same is t and np.array_equal(t.cpu().numpy(), want), (name, conn, min_area)


def test_remove_small_other_dtypes_fill_and_background_none():
    a, dims = C.CASES["noise4_wide"]
    for dtype in (torch.int16, torch.int32, torch.int64):
        t = torch.from_numpy(a.astype(NP[dtype])).to(DEV)
        want = C.remove_small(a, dims, 4, 3, background=None, fill=7)
        got = remove_small_components(t, 3, connectivity=4, background=None, fill=7)
        assert np.array_equal(got.cpu().numpy(), want)
    b = torch.from_numpy(a != 0).to(DEV)
    want = C.remove_small(a != 0, dims, 8, 4)
    assert np.array_equal(remove_small_components(b, 4).cpu().numpy(), want)


def test_rle_of_the_cleaned_map():
    a, dims = C.CASES["blobs_wide"]
    t = torch.from_numpy(a).to(DEV)
    want = torch.from_numpy(C.remove_small(a, dims, 8, 30)).to(DEV)
    got = rle_encode_device(remove_small_components(t, min_area=30, connectivity=8), labels=range(6))
    for g, w in zip(got, rle_encode_device(want, labels=range(6))):
        assert torch.equal(g, w)


@pytest.mark.parametrize("name", C.BIG_CASES)
def test_two_runs_are_bit_identical(name):
    t, dims = _dev(name, torch.uint8)
    for conn in C.CONNECTIVITIES[dims]:
        cc1, n1 = _label(t, connectivity=conn)
        cc2, n2 = _label(t, connectivity=conn)
        assert torch.equal(cc1, cc2) and torch.equal(n1, n2)
        assert torch.equal(remove_small_components(t, 64, connectivity=conn), remove_small_components(t, 64, connectivity=conn))


def test_non_default_stream_and_non_contiguous_input():
    a, dims = C.CASES["blobs"]
    t = torch.from_numpy(a).to(DEV)
    cc, count = _label(t)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        cc_s, count_s = _label(t)
        clean_s = remove_small_components(t, 5)
    torch.cuda.current_stream(DEV).wait_stream(stream)
    assert torch.equal(cc_s, cc) and torch.equal(count_s, count) and torch.equal(clean_s, remove_small_components(t, 5))
    wide = torch.from_numpy(np.ascontiguousarray(a.T)).to(DEV).t()                       # the same map with other strides
    assert not wide.is_contiguous()
    cc_t, count_t = _label(wide)
    assert torch.equal(cc_t, cc) and torch.equal(count_t, count)
    assert torch.equal(remove_small_components(wide, 5), remove_small_components(t, 5))
    every_other = torch.from_numpy(np.repeat(a, 2, axis=1)).to(DEV)[:, ::2]
    assert not every_other.is_contiguous() and torch.equal(_label(every_other)[0], cc)


def test_empty_inputs_launch_nothing():
    before = N.calls
    cc, count = connected_components(torch.zeros((0, 5), dtype=torch.uint8, device=DEV))
    assert cc.shape == (0, 5) and cc.dtype == torch.int32 and int(count) == 0
    cc, count = connected_components(torch.zeros((0, 4, 5), dtype=torch.uint8, device=DEV))
    assert cc.shape == (0, 4, 5) and count.shape == (0,)
    assert remove_small_components(torch.zeros((3, 0), dtype=torch.uint8, device=DEV), 4).shape == (3, 0)
    assert component_stats(torch.zeros((4, 4), dtype=torch.int32, device=DEV), max_components=0)["area"].shape == (0,)
    assert N.calls == before
