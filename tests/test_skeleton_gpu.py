"""GPU: the thinning kernels (csrc/ptb_skeleton.hip) against the direct model of tests/skeleton_cases.py and against the host form, bit for
bit, on every case and both methods, with the model's iteration count; run-to-run identity; every base one element into its buffer (the
peeled loads), every label dtype, other strides, out= (direct, misaligned, the input itself), a caller's stream, one native call per
public call, max_iterations that cut a launch short; centerline_dice with three classes on a stack of two against the model."""
import numpy as np
import pytest
import torch

import skeleton_cases as SC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import centerline_dice, skeletonize

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LABEL_DTYPES = (torch.bool, torch.uint8, torch.int16, torch.int32, torch.int64)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _offset(t):
    """a contiguous device copy of ``t`` that starts one element into its buffer"""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and (view.data_ptr() % 16 != 0 or t.numel() == 0)
    return view


def _run(x, **kw):
    before = N.calls
    got, n = skeletonize(x, return_iterations=True, **kw)
    assert N.calls == before + 1, "one native call per public call"
    assert got.shape == x.shape and got.device == x.device
    return got, n


@pytest.mark.parametrize("method", SC.METHODS)
@pytest.mark.parametrize("name", SC.NAMES)
def test_kernels_equal_the_model_and_the_host_form(name, method):
    mask = SC.CASES[name]
    want, iterations = SC.expected(name, method)
    x = _dev(mask)
    got, n = _run(x, method=method)
    assert got.dtype == torch.bool
    assert np.array_equal(got.cpu().numpy(), want), (name, method, "model")
    assert torch.equal(got.cpu(), skeletonize(x.cpu(), method=method)), (name, method, "host form")
    assert n == iterations, (name, method, n, iterations)
    if name == "three_batches":                                                # more sub-iterations than two read-back batches of launches hold
        assert 2 * (iterations - 1) >= 2 * SC.RELAX_BATCH * SC.STEPS
    again, n2 = _run(x, method=method)                                         # two runs: the same bits
    assert torch.equal(again, got) and n2 == n
    off, n3 = _run(_offset(x), method=method)                                  # the peeled loads
    assert torch.equal(off, got) and n3 == n


@pytest.mark.parametrize("dtype", LABEL_DTYPES, ids=str)
def test_every_label_dtype_and_object_rule(dtype):
    """33 x 110 int16 rows are no multiple of 16 bytes: peeled; 64 x 64: the 16-byte loads; and each again from a base one element in"""
    for name in ("border_33x110", "border_64x64"):
        mask = SC.CASES[name]
        classes = mask * np.random.default_rng(2).integers(1, 4, mask.shape)
        for place in (lambda t: t, _offset):
            if dtype == torch.bool:
                x = place(_dev(mask))
                assert torch.equal(skeletonize(x).cpu(), skeletonize(x.cpu()))
                assert torch.equal(skeletonize(x, foreground=0).cpu(), skeletonize(x.cpu(), foreground=0))
                assert not skeletonize(x, foreground=2).any()
                continue
            x = place(_dev(classes, dtype))
            for kw in (dict(), dict(foreground=2), dict(background=3), dict(foreground=1 << 40), dict(background=-(1 << 40))):
                assert torch.equal(skeletonize(x, **kw).cpu(), skeletonize(x.cpu(), **kw)), (name, dtype, kw)


@pytest.mark.parametrize("method", SC.METHODS)
def test_max_iterations_cut_a_launch_short(method):
    x = _dev(SC.CASES["full"])
    for n in (0, 1, 3, SC.STEPS // 2, SC.STEPS // 2 + 3, 21):                  # 3, 19 and 21 are no multiple of STEPS / 2
        want, took = SC.expected("full", method, n)
        got, t = _run(x, method=method, max_iterations=n)
        assert np.array_equal(got.cpu().numpy(), want) and t == took == n, (method, n, t)
    want, took = SC.expected("full", method)
    got, t = _run(x, method=method, max_iterations=took + 1)                   # the cut behind the last iteration that deletes
    assert np.array_equal(got.cpu().numpy(), want) and t == took
    got, t = _run(x, method=method, max_iterations=10 ** 9)                    # beyond the guard: to stability
    assert np.array_equal(got.cpu().numpy(), want) and t == took


def test_out_streams_and_strides():
    mask = SC.CASES["retire"]
    want = torch.from_numpy(SC.expected("retire", "guo_hall")[0].copy())
    x = _dev(mask)
    for dtype in (torch.bool, torch.uint8):
        out = torch.full(mask.shape, 1, dtype=dtype, device=DEV)
        before = N.calls
        assert skeletonize(x, out=out) is out and torch.equal(out.cpu().bool(), want) and N.calls == before + 1
        off = _offset(torch.zeros(mask.shape, dtype=dtype, device=DEV))         # a misaligned out
        assert skeletonize(x, out=off) is off and torch.equal(off.cpu().bool(), want)
    own = x.clone()                                                            # out is the input itself
    assert skeletonize(own, out=own) is own and torch.equal(own.cpu(), want)
    own = x.to(torch.uint8)
    assert skeletonize(own, out=own) is own and torch.equal(own.cpu().bool(), want)
    stream = torch.cuda.Stream(device=DEV)                                     # a stream of the caller's
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        got = skeletonize(x)
    stream.synchronize()
    assert torch.equal(got.cpu(), want)
    turned = x.t().contiguous().t()                                            # other strides are copied first
    assert not turned.is_contiguous() and torch.equal(skeletonize(turned).cpu(), want)
    wide = torch.zeros((mask.shape[0], 2 * mask.shape[1]), dtype=torch.bool, device=DEV)
    wide[:, ::2] = x
    assert torch.equal(skeletonize(wide[:, ::2]).cpu(), want)
    before = N.calls                                                           # empty inputs launch nothing
    empty, n = skeletonize(torch.zeros((3, 0, 5), dtype=torch.int32, device=DEV), return_iterations=True)
    assert empty.shape == (3, 0, 5) and empty.dtype == torch.bool and empty.device == DEV and n == 0 and N.calls == before


@pytest.mark.parametrize("method", SC.METHODS)
def test_centerline_dice_three_classes_on_a_stack_of_two(method):
    rng = np.random.default_rng(9)
    truth = np.stack([SC.CASES["blobs"][:70, :100], SC.CASES["blobs"][70:140, 60:160]]) * rng.integers(1, 4, (2, 70, 100))
    pred = np.roll(truth, (2, -3), (-2, -1))
    pred[1][pred[1] == 3] = 0
    for values, kinds in (([1, 2, 3], (torch.uint8, torch.int64)), (None, (torch.int16, torch.int16)), ([3, 9], (torch.int32, torch.uint8))):
        want = SC.cldice_model(pred, truth, values, method)
        p, t = _dev(pred, kinds[0]), _dev(truth, kinds[1])
        before = N.calls
        got = centerline_dice(p, t, labels=values, method=method)
        assert N.calls == before + 1
        K = 1 if values is None else len(values)
        assert got["counts"].dtype == torch.int64 and got["counts"].shape == (2, K, 4) and got["counts"].device == DEV
        assert np.array_equal(got["counts"].cpu().numpy(), want[0]), (method, values)
        host = centerline_dice(p.cpu(), t.cpu(), labels=values, method=method)
        for key, w in zip(("cldice", "tprec", "tsens"), want[1:]):
            assert got[key].dtype == torch.float32 and got[key].shape == (2, K)
            np.testing.assert_allclose(got[key].cpu().numpy(), w, rtol=1e-6, atol=0, equal_nan=True)
            assert torch.equal(got[key].cpu().view(torch.int32), host[key].view(torch.int32)), key       # the host form: the same bits
        again = centerline_dice(_offset(p), _offset(t), labels=values, method=method)
        assert all(torch.equal(again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k],
                               got[k].view(torch.int32) if got[k].dtype == torch.float32 else got[k]) for k in got)
    same = centerline_dice(_dev(truth), _dev(truth), labels=[1, 2, 3])
    assert (same["cldice"] == 1).all()
    with pytest.raises(ValueError, match="needs a workspace of"):
        centerline_dice(_dev(truth), _dev(truth), max_workspace_bytes=100)
