"""GPU: the watershed kernels (csrc/ptb_watershed.hip) against the two-search model of tests/watershed_cases.py and against the host form:
labels, pass height and seed, bit for bit, on every case and connectivity; every height and marker element type in the wide and the
peeled load arm; out=, streams, strides, empty inputs, one native call per public call, run-to-run identity; the sweep loop across more
than one batch, and its bound as a clean exception."""
import numpy as np
import pytest
import torch

import watershed_cases as WC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import watershed

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BATCH = 8                                  # RELAX_BATCH of csrc/ptb_relax_device.h: the sweeps between two read-backs
HEIGHT_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.uint8, torch.int16)
MARKER_DTYPES = (torch.bool, torch.uint8, torch.int16, torch.int32, torch.int64)


def _offset(t):
    """a contiguous device copy of ``t`` that starts one element into its buffer: the peeled loads"""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def _tensors(case, place=lambda t: t.to(DEV)):
    return place(torch.from_numpy(case.height)), place(torch.from_numpy(case.markers)), None if case.mask is None else place(torch.from_numpy(case.mask))


def _run(h, m, mask, case, connectivity, **kw):
    before = N.calls
    got = watershed(h, m, mask=mask, connectivity=connectivity, background=case.background, dims=case.dims, return_cost=True, return_seed=True, return_sweeps=True, **kw)
    assert N.calls == before + 1, "one native call per public call"
    assert got[0].dtype == m.dtype and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
    assert all(t.shape == m.shape and t.device == DEV for t in got[:3])
    return got


def _same(got, labels, cost, seed, what):
    assert np.array_equal(got[0].cpu().numpy(), labels), (what, "labels")
    assert np.array_equal(got[1].cpu().numpy().view(np.int32), cost.view(np.int32)), (what, "cost")
    assert np.array_equal(got[2].cpu().numpy(), seed), (what, "seed")


@pytest.mark.parametrize("name,connectivity", WC.PAIRS)
def test_kernels_equal_the_model_and_the_host_form(name, connectivity):
    case = WC.CASES[name]
    got = _run(*_tensors(case), case, connectivity)
    _same(got, *case.expected(connectivity), name)
    h, m, mask = _tensors(case, lambda t: t)
    host = watershed(h, m, mask=mask, connectivity=connectivity, background=case.background, dims=case.dims, return_cost=True, return_seed=True)
    _same(got, host[0].numpy(), host[1].numpy(), host[2].numpy(), (name, "host form"))
    assert got[3][0] >= 1 and got[3][1] >= 1
    again = _run(*_tensors(case), case, connectivity)                          # two runs: the same bits (the sweeps may differ: a halo read may see this sweep's value)
    assert all(torch.equal(a, b) for a, b in zip(got[:3], again[:3]))
    plain = watershed(*_tensors(case)[:2], mask=_tensors(case)[2], connectivity=connectivity, background=case.background, dims=case.dims)
    assert torch.equal(plain, got[0])                                          # (no optional output: other flags)


@pytest.mark.parametrize("name", ("u8_noise_holes", "odd_width", "volume_stack"))
def test_every_element_type_in_both_load_arms(name):
    """u8_noise_holes: every value is exact in every height type; 9900 positions, aligned: the wide arm.  odd_width: 1961 positions:
    peeled.  Every case again from a base one element into its buffer: peeled, misaligned."""
    case = WC.CASES[name]
    conn = WC.CONNECTIVITIES[case.dims][1]
    h0 = torch.from_numpy(case.height)
    if h0.dtype != torch.uint8:                                                # values every height type holds exactly
        h0 = (h0 * 40).round().clamp(-100, 100).to(torch.int16)
    m0 = torch.from_numpy(case.markers)
    mask = None if case.mask is None else torch.from_numpy(case.mask)
    want = watershed(h0.float(), m0, mask=mask, connectivity=conn, dims=case.dims, return_cost=True, return_seed=True)
    refs = {md: watershed(h0.float(), m0.to(md), mask=mask, connectivity=conn, dims=case.dims, return_seed=True) for md in MARKER_DTYPES}
    for place in (lambda t: t.to(DEV), _offset):
        for hd in HEIGHT_DTYPES:
            if hd == torch.uint8 and h0.dtype != torch.uint8:
                continue
            got = _run(place(h0.to(hd)), place(m0), None if mask is None else place(mask), case, conn)
            _same(got, want[0].numpy(), want[1].numpy(), want[2].numpy(), (name, hd))
        for md in MARKER_DTYPES:
            got = _run(place(h0.float()), place(m0.to(md)), None if mask is None else place(mask.to(torch.uint8) * 3), case, conn)
            assert torch.equal(got[0].cpu(), refs[md][0]) and torch.equal(got[2].cpu(), refs[md][1]), (name, md)


@pytest.mark.parametrize("name", ("blobs_edt", "volume"))
def test_out_streams_and_strides(name):
    case = WC.CASES[name]
    conn = WC.CONNECTIVITIES[case.dims][1]
    labels = case.expected(conn)[0]
    h, m, mask = _tensors(case)
    kw = dict(mask=mask, connectivity=conn, dims=case.dims)
    out = torch.full_like(m, 77)
    before = N.calls
    assert watershed(h, m, out=out, **kw) is out and np.array_equal(out.cpu().numpy(), labels) and N.calls == before + 1
    own = m.clone()                                                            # out may be the markers themselves
    assert watershed(h, own, out=own, **kw) is own and np.array_equal(own.cpu().numpy(), labels)
    off = _offset(torch.zeros_like(m))                                         # a misaligned out
    assert watershed(h, m, out=off, **kw) is off and np.array_equal(off.cpu().numpy(), labels)
    stream = torch.cuda.Stream(device=DEV)                                     # a stream of the caller's
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        got = watershed(h, m, **kw)
    stream.synchronize()
    assert np.array_equal(got.cpu().numpy(), labels)
    # other strides are copied first: a map held transposed, and every other column of a wider one
    ht, mt, kt = (t.transpose(-1, -2).contiguous().transpose(-1, -2) for t in (h, m, mask))
    assert not mt.is_contiguous() and np.array_equal(watershed(ht, mt, mask=kt, connectivity=conn, dims=case.dims).cpu().numpy(), labels)
    wide = torch.zeros(m.shape[:-1] + (2 * m.shape[-1],), dtype=m.dtype, device=DEV)
    wide[..., ::2] = m
    assert np.array_equal(watershed(h, wide[..., ::2], **kw).cpu().numpy(), labels)


def test_empty_inputs_launch_nothing():
    before = N.calls
    got = watershed(torch.zeros((3, 0, 5), device=DEV), torch.zeros((3, 0, 5), dtype=torch.int16, device=DEV), return_cost=True, return_seed=True, return_sweeps=True)
    assert got[0].shape == (3, 0, 5) and got[0].dtype == torch.int16 and got[0].device == DEV and got[3] == (0, 0)
    assert N.calls == before


def test_long_serpentine_takes_more_sweeps_than_a_batch_and_max_sweeps_bounds_them():
    case = WC.CASES["serpentine_long"]
    h, m, mask = _tensors(case)
    got = _run(h, m, mask, case, 4)
    _same(got, *case.expected(4), "serpentine_long")
    assert got[3][0] > BATCH and got[3][1] > BATCH, got[3]
    before = N.calls
    with pytest.raises(RuntimeError, match=r"phase 1 \(the cost relaxation\) did not converge within max_sweeps=1: 1 sweeps run"):
        watershed(h, m, mask=mask, connectivity=4, max_sweeps=1)
    with pytest.raises(RuntimeError, match=r"phase 1 \(the cost relaxation\) did not converge within max_sweeps=9: 9 sweeps run"):
        watershed(h, m, mask=mask, connectivity=4, max_sweeps=BATCH + 1)       # (a second, shorter batch)
    assert N.calls == before + 2
    again = _run(h, m, mask, case, 4)                                          # the process goes on
    assert torch.equal(again[0], got[0])
