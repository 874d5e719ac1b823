"""GPU: the reconstruction kernels (csrc/ptb_reconstruct.hip) against the textbook model of tests/reconstruct_cases.py and against the host
form, bit for bit, on every case and connectivity; every value dtype in the wide and the peeled load arm and from a base one element into
its buffer; out= (an input, a misaligned one), a caller's stream, strides, empty inputs, one native call per public call, run-to-run
identity; the sweep loop across more than one batch, and its bound as a clean exception."""
import numpy as np
import pytest
import torch

import reconstruct_cases as RC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import fill_holes, h_maxima, h_minima, reconstruction, regional_maxima, regional_minima
from test_reconstruct_cpu import call

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BATCH = 8                                  # RELAX_BATCH of csrc/ptb_relax_device.h: the sweeps between two read-backs
DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.uint8, torch.int16)


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _offset(t):
    """a contiguous device copy of ``t`` that starts one element into its buffer: the peeled loads"""
    t = (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).to(DEV)
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def _run(case, connectivity, place=_dev, **kw):
    before = N.calls
    got, sweeps = call(case, connectivity, place, return_sweeps=True, **kw)
    assert N.calls == before + 1, "one native call per public call"
    assert got.shape == case.image.shape and got.device == DEV
    return got, sweeps


@pytest.mark.parametrize("name,connectivity", RC.PAIRS)
def test_kernels_equal_the_model_and_the_host_form(name, connectivity):
    case = RC.CASES[name]
    got, sweeps = _run(case, connectivity)
    assert RC.same_bits(got.cpu().numpy(), case.expected(connectivity)), (name, "model")
    assert RC.same_bits(got.cpu().numpy(), call(case, connectivity).numpy()), (name, "host form")
    assert sweeps[0] >= 1 and (sweeps[1] >= 1) == (case.op == "h"), sweeps
    again, _ = _run(case, connectivity)                                        # two runs: the same bits (the sweeps may differ: a halo read may see this sweep's value)
    assert RC.same_bits(again.cpu().numpy(), got.cpu().numpy())
    off, _ = _run(case, connectivity, _offset)                                 # every base one element into its buffer: the peeled arm
    assert RC.same_bits(off.cpu().numpy(), got.cpu().numpy())


@pytest.mark.parametrize("name", ("wide/h_maxima", "odd_total/h_maxima", "volume_stack/h_maxima"))
def test_every_dtype_in_both_load_arms(name):
    """wide: 9984 positions, aligned: the wide arm.  odd_total: 1961 positions: peeled.  Every case again from a base one element into its
    buffer: peeled, misaligned.  Values scaled by 40 are small integers: every dtype holds them exactly."""
    case = RC.CASES[name]
    conn = RC.CONNECTIVITIES[case.dims][1]
    img = torch.from_numpy(np.round(case.image * 40).astype(np.int16))
    img = img - img.min() + 3                                                  # (uint8 holds them too)
    assert 0 <= int(img.min()) and int(img.max()) <= 200
    seed = (img - 4).clamp(min=0)
    dom = torch.from_numpy(np.random.default_rng(5).random(case.image.shape) >= 0.1)
    kw = dict(connectivity=conn, dims=case.dims)
    want = dict(hmax=h_maxima(img.float(), 4.0, **kw), hmin=h_minima(img.float(), 3.0, domain=dom, **kw), rmax=regional_maxima(img.float(), domain=dom, **kw),
                rmin=regional_minima(img.float(), **kw), dil=reconstruction(seed.float(), img.float(), domain=dom, **kw),
                ero=reconstruction((img + 5).float(), img.float(), method="erosion", **kw), fill=fill_holes(img.float(), domain=dom, **kw))
    for place in (lambda t: t.to(DEV), _offset):
        for dt in DTYPES:
            x, s, s2, k = place(img.to(dt)), place(seed.to(dt)), place((img + 5).to(dt)), place(dom)
            before = N.calls
            got = dict(hmax=h_maxima(x, 4.0, **kw), hmin=h_minima(x, 3.0, domain=k, **kw), rmax=regional_maxima(x, domain=k, **kw), rmin=regional_minima(x, **kw),
                       dil=reconstruction(s, x, domain=k, **kw), ero=reconstruction(s2, x, method="erosion", **kw), fill=fill_holes(x, domain=k, **kw))
            assert N.calls == before + len(got)
            for key, g in got.items():
                w = want[key] if want[key].dtype == torch.bool else want[key].to(dt)
                assert g.dtype == w.dtype and torch.equal(g.cpu(), w), (name, dt, key)
    mask = img > int(img.median())                                             # bool and uint8 masks of hole filling
    for place in (lambda t: t.to(DEV), _offset):
        for m in (mask, mask.to(torch.uint8)):
            got = fill_holes(place(m), domain=place(dom), **kw)
            assert got.dtype == m.dtype and torch.equal(got.cpu(), fill_holes(m, domain=dom, **kw)), (name, m.dtype)


@pytest.mark.parametrize("name", ("blobs/dilation", "volume_stack/dilation"))
def test_out_streams_and_strides(name):
    case = RC.CASES[name]
    conn = RC.CONNECTIVITIES[case.dims][1]
    want = torch.from_numpy(case.expected(conn).copy())
    peaks = torch.from_numpy(RC.Case("x", "h", case.image, domain=case.domain, h=0.5, dims=case.dims).expected(conn).copy())
    seed, mask, dom = _dev(case.seed), _dev(case.image), None if case.domain is None else _dev(case.domain)
    kw = dict(connectivity=conn, domain=dom, dims=case.dims)
    out = torch.full_like(mask, 77)
    before = N.calls
    assert reconstruction(seed, mask, out=out, **kw) is out and torch.equal(out.cpu(), want) and N.calls == before + 1
    own = seed.clone()                                                         # out may be an input: the seed, the mask
    assert reconstruction(own, mask, out=own, **kw) is own and torch.equal(own.cpu(), want)
    own = mask.clone()
    assert reconstruction(seed, own, out=own, **kw) is own and torch.equal(own.cpu(), want)
    off = _offset(torch.zeros_like(mask))                                      # a misaligned out
    assert reconstruction(seed, mask, out=off, **kw) is off and torch.equal(off.cpu(), want)
    flags = torch.zeros(mask.shape, dtype=torch.bool, device=DEV)
    assert h_maxima(mask, 0.5, out=flags, **kw) is flags and torch.equal(flags.cpu(), peaks)
    off = _offset(torch.zeros(mask.shape, dtype=torch.bool))
    assert h_maxima(mask, 0.5, out=off, **kw) is off and torch.equal(off.cpu(), peaks)
    stream = torch.cuda.Stream(device=DEV)                                     # a stream of the caller's
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        got = reconstruction(seed, mask, **kw)
        got2 = h_maxima(mask, 0.5, **kw)
    stream.synchronize()
    assert torch.equal(got.cpu(), want) and torch.equal(got2.cpu(), peaks)
    # other strides are copied first: maps held transposed, and every other column of a wider one
    turned = [None if t is None else t.transpose(-1, -2).contiguous().transpose(-1, -2) for t in (seed, mask, dom)]
    assert not turned[1].is_contiguous()
    assert torch.equal(reconstruction(turned[0], turned[1], connectivity=conn, domain=turned[2], dims=case.dims).cpu(), want)
    wide = torch.zeros(mask.shape[:-1] + (2 * mask.shape[-1],), dtype=mask.dtype, device=DEV)
    wide[..., ::2] = mask
    assert torch.equal(reconstruction(seed, wide[..., ::2], **kw).cpu(), want) and torch.equal(h_maxima(wide[..., ::2], 0.5, **kw).cpu(), peaks)


def test_empty_inputs_launch_nothing():
    before = N.calls
    got, sweeps = h_maxima(torch.zeros((3, 0, 5), device=DEV), 1.0, return_sweeps=True)
    assert got.shape == (3, 0, 5) and got.dtype == torch.bool and got.device == DEV and sweeps == (0, 0)
    empty = torch.zeros((0, 2, 2), dtype=torch.int16, device=DEV)
    assert reconstruction(empty, empty, dims=3).shape == (0, 2, 2) and fill_holes(empty.to(torch.bool)).dtype == torch.bool
    assert N.calls == before


def test_long_serpentine_takes_more_sweeps_than_a_batch_and_max_sweeps_bounds_them():
    case = RC.CASES["serpentine_long/dilation"]
    got, sweeps = _run(case, 4)
    assert RC.same_bits(got.cpu().numpy(), case.expected(4))
    assert sweeps[0] > BATCH and sweeps[1] == 0, sweeps
    before = N.calls
    with pytest.raises(RuntimeError, match=r"phase 1 \(the reconstruction relaxation\) did not converge within max_sweeps=1: 1 sweeps run"):
        call(case, 4, _dev, max_sweeps=1)
    with pytest.raises(RuntimeError, match=r"phase 1 \(the reconstruction relaxation\) did not converge within max_sweeps=9: 9 sweeps run"):
        call(case, 4, _dev, max_sweeps=BATCH + 1)                              # (a second, shorter batch)
    assert N.calls == before + 2
    again, _ = _run(case, 4)                                                   # the process goes on
    assert torch.equal(again, got)
    # ... and the second phase of the h-maxima names itself: with h = 0 the first phase starts at its fixed point (one sweep that changes
    # nothing); in the second the one higher position at the start of the corridor has to raise the whole corridor behind it
    peak = _dev(np.where(case.seed != 0, np.float32(3.0), case.image))
    with pytest.raises(RuntimeError, match=r"phase 2 \(the regional-extrema relaxation\) did not converge within max_sweeps=2: 2 sweeps run"):
        h_maxima(peak, 0.0, connectivity=4, domain=_dev(case.domain), max_sweeps=2)
    flags, sweeps = h_maxima(peak, 0.0, connectivity=4, domain=_dev(case.domain), return_sweeps=True)
    assert sweeps[0] == 1 and sweeps[1] > BATCH and int(flags.sum()) == 1 and bool(flags[0, 0])
