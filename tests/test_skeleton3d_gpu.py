"""GPU: the 3-D thinning kernel (csrc/ptb_skeleton3d.hip) against the direct model of tests/skeleton3d_cases.py and against the host form, bit
for bit, on every case with the model's iteration count; run-to-run identity; a base one element into its buffer; every label dtype with
foreground=; out= being the input; max_iterations that cut the launches short; one native call per public call; centerline_dice(dims=3)
against the CPU result."""
import numpy as np
import pytest
import torch

import skeleton3d_cases as SC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import centerline_dice, skeletonize
from test_skeleton_gpu import DEV, LABEL_DTYPES, _dev, _offset

pytestmark = pytest.mark.gpu


def _run(x, **kw):
    before = N.calls
    got, n = skeletonize(x, dims=3, return_iterations=True, **kw)
    assert N.calls == before + 1, "one native call per public call"
    assert got.shape == x.shape and got.device == x.device and got.dtype == torch.bool
    return got, n


@pytest.mark.parametrize("name", SC.NAMES)
def test_kernel_equals_the_model_and_the_host_form(name):
    want, iterations = SC.expected(name)
    x = _dev(SC.CASES[name])
    got, n = _run(x)
    assert np.array_equal(got.cpu().numpy(), want), (name, "model")
    assert torch.equal(got.cpu(), skeletonize(x.cpu(), dims=3)), (name, "host form")
    assert n == iterations, (name, n, iterations)
    again, n2 = _run(x)                                                        # two runs: the same bits
    assert torch.equal(again, got) and n2 == n
    off, n3 = _run(_offset(x))                                                 # the peeled loads
    assert torch.equal(off, got) and n3 == n


@pytest.mark.parametrize("dtype", LABEL_DTYPES, ids=str)
def test_every_label_dtype_with_foreground(dtype):
    mask = SC.CASES["faces_9x10x33"]
    if dtype == torch.bool:
        x = _dev(mask)
        assert torch.equal(skeletonize(x, foreground=0, dims=3).cpu(), skeletonize(x.cpu(), foreground=0, dims=3))
        assert not skeletonize(x, foreground=2, dims=3).any()
        return
    x = _dev(mask * np.random.default_rng(2).integers(1, 4, mask.shape), dtype)
    for kw in (dict(foreground=2), dict(background=3), dict(foreground=1 << 40)):
        assert torch.equal(skeletonize(x, dims=3, **kw).cpu(), skeletonize(x.cpu(), dims=3, **kw)), (dtype, kw)


def test_out_is_the_input_and_max_iterations_cut_the_launches():
    want = torch.from_numpy(SC.expected("seam")[0].copy())
    for own in (_dev(SC.CASES["seam"]), _dev(SC.CASES["seam"], torch.uint8)):
        assert skeletonize(own, out=own, dims=3) is own and torch.equal(own.cpu().bool(), want)
    x = _dev(SC.CASES["box"])
    full, took = SC.expected("box")
    for n in (0, 1, took + 1, 10 ** 9):                                        # the cut, the cut behind the last iteration that deletes, beyond the guard
        want, count = SC.expected("box", n)
        got, t = _run(x, max_iterations=n)
        assert np.array_equal(got.cpu().numpy(), want) and t == count == min(n, took), (n, t)
    before = N.calls                                                           # empty inputs launch nothing
    assert skeletonize(torch.zeros((3, 0, 5, 4), dtype=torch.int32, device=DEV), dims=3).shape == (3, 0, 5, 4) and N.calls == before


def test_centerline_dice_equals_the_cpu_result():
    truth = SC.CASES["stack"] * np.random.default_rng(1).integers(1, 3, SC.CASES["stack"].shape)
    pred = np.roll(truth, (1, -2), (-2, -1))
    pred[1][pred[1] == 2] = 0
    for values, kinds in (([1, 2], (torch.uint8, torch.int64)), (None, (torch.int16, torch.int32))):
        p, t = _dev(pred, kinds[0]), _dev(truth, kinds[1])
        before = N.calls
        got = centerline_dice(p, t, labels=values, dims=3)
        assert N.calls == before + 1
        host = centerline_dice(p.cpu(), t.cpu(), labels=values, dims=3)
        assert got["counts"].dtype == torch.int64 and got["counts"].device == DEV and torch.equal(got["counts"].cpu(), host["counts"])
        for key in ("cldice", "tprec", "tsens"):
            assert got[key].dtype == torch.float32 and torch.equal(got[key].cpu().view(torch.int32), host[key].view(torch.int32)), key
