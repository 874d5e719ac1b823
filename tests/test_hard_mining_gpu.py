"""GPU: the hard-example-mining kernels (csrc/ptb_hard_mining.hip) against the float64 model of tests/hard_mining_cases.py.

  loss, thr  within seg_loss_cases.TOL (rtol 1e-5, atol 1e-5) of the model; the kept count exactly.
  gradient   within GRAD_TOL (rtol 2e-4), atol 2e-6 * |coef| / kept; an UNDECIDED element of a tie-free case (float64 loss within
             TOL["rtol"] * max(1, thr) of the model's thr) may have the gradient of either decision -- hard_mining_cases.check.
  ties       the weights the gradient implies within TOL of the model's: kept / n with all vectors identical, (kept - gt) / eq inside a group.
  bits       a second run of forward and backward changes no bit of loss, thr and gradient.
  calls      one native call per forward and one per backward."""
import numpy as np
import pytest
import torch

import hard_mining_cases as HC
import seg_loss_cases as SC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd import losses
from pytorch_toolbelt_amd.losses import _kernels as K

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _run(name, **extra):
    before = N.calls
    out = HC.run(name, losses.topk_cross_entropy, losses.ohem_cross_entropy, device=DEV, **extra)
    assert N.calls == before + 2, "one native call per forward, one per backward"
    return out


@pytest.fixture(scope="module")
def results():
    """every case once on the device: (loss, thr, kept, grad)"""
    return {name: _run(name) for name in HC.CASES}


@pytest.mark.parametrize("name", list(HC.CASES))
def test_loss_threshold_count_and_gradient_against_the_model(name, results):
    loss, thr, kept, grad = results[name]
    assert loss.is_cuda and thr.is_cuda and kept.is_cuda
    HC.check(name, loss, thr, kept, grad)


@pytest.mark.parametrize("name", HC.TIE_CASES)
def test_tie_weights(name, results):
    want = HC.model(name)
    got = HC.weights_from_gradient(name, results[name][3])
    known = ~np.isnan(got)
    assert known.mean() > 0.3, name
    err = np.abs(got - want.weight)[known]
    print(f"{name}: weights {np.unique(np.round(want.weight, 6))}, worst error {err.max():.3e}")
    assert (err <= SC.TOL["rtol"] * want.weight[known] + SC.TOL["atol"]).all()


def test_second_run_changes_no_bit(results):
    for name in ("s3077", "s4096_per_sample", "c17", "c16_wide", "multilabel_per_sample", "k1", "ohem_above", "ohem_per_sample", "ignore_wide", "tie_groups_c17",
                 "extreme_c19"):
        again = _run(name)
        for a, b in zip(results[name], again):
            assert torch.equal(a, b), name


@pytest.mark.parametrize("name", ("s1027_per_sample", "s4096_per_sample", "multilabel_per_sample", "ohem_per_sample", "ohem_ignore_sample", "ignore_wide",
                                  "tie_groups_c17"))
def test_per_sample_is_the_samples_one_by_one(name, results):
    case = HC.CASES[name]
    x, t = HC.inputs(name)
    fn = losses.topk_cross_entropy if case.rule == "topk" else losses.ohem_cross_entropy
    kw = HC.arguments(case)
    kw.update(per_sample=False, reduction="mean")
    coef = torch.from_numpy(HC.model(name).coef).to(DEV, torch.float32)
    loss, thr, kept, grad = results[name]
    for b in range(case.B):
        xb = torch.from_numpy(x[b:b + 1].copy()).to(DEV).requires_grad_(True)
        lb, tb, kb = fn(xb, torch.from_numpy(t[b:b + 1].copy()).to(DEV), return_threshold=True, **kw)
        (lb * coef[b]).backward()
        assert torch.equal(lb, loss[b]) and torch.equal(tb, thr[b]) and torch.equal(kb, kept[b]), (name, b)
        # (a sample whose start is not 16-byte aligned inside the batch takes the peeled kernel there: the same arithmetic)
        assert torch.equal(xb.grad[0], grad[b]), (name, b)


@pytest.mark.parametrize("name", ("s1023", "s4096", "c9", "c19", "binary_s1024", "multilabel_s1027", "k50_per_sample", "ohem_floor", "ohem_equal", "ignore",
                                  "tie_groups_easy", "tie_identical_binary"))
def test_device_against_host_form(name, results):
    host = HC.run(name, losses.topk_cross_entropy, losses.ohem_cross_entropy)
    loss, thr, kept, grad = results[name]
    assert torch.equal(kept.cpu(), host[2])
    torch.testing.assert_close(loss.cpu(), host[0], rtol=SC.TOL["rtol"], atol=SC.TOL["atol"])
    torch.testing.assert_close(thr.cpu(), host[1], rtol=SC.TOL["rtol"], atol=SC.TOL["atol"])
    want = HC.model(name)
    bound = SC.GRAD_TOL["rtol"] * np.abs(want.grad) + SC.GRAD_TOL["atol"] * want.scale
    off = (np.abs(grad.cpu().numpy() - host[3].numpy()) > 2 * bound) & ~(want.undecided & (not HC.CASES[name].ties))
    assert not off.any(), (name, int(off.sum()))


def test_bad_label_surfaces_through_check_labels():
    x, t = HC.inputs("c5")
    xt, tt = torch.from_numpy(x.copy()).to(DEV), torch.from_numpy(t.copy()).to(DEV)
    bad = tt.clone()
    bad[0, 2, 3] = 5 + 4
    K.flush_label_check()
    for fn in (losses.topk_cross_entropy, losses.ohem_cross_entropy):
        poisoned = fn(xt, bad)
        with pytest.raises(RuntimeError, match="Class values must be smaller"):
            K.flush_label_check()
        assert torch.isnan(poisoned)                                            # never a finite loss from a bad label
        assert torch.isfinite(fn(xt, bad, ignore_index=5 + 4))
        assert torch.isfinite(fn(xt, tt))
        K.flush_label_check()


def test_non_contiguous_and_half_logits_are_their_widened_copy():
    for name in ("s1024", "c9", "multilabel_s1024"):
        case = HC.CASES[name]
        x, t = HC.inputs(name)
        fn = losses.topk_cross_entropy
        kw = HC.arguments(case)
        tt = torch.from_numpy(t.copy()).to(DEV)
        xt = torch.from_numpy(x.copy()).to(DEV)
        last = xt.movedim(1, -1).contiguous().movedim(-1, 1)                    # channels-last memory
        assert not last.is_contiguous() or case.C == 1
        for view in (last, xt.half(), xt.bfloat16()):
            a = view.detach().clone().requires_grad_(True) if view is not last else last.detach().requires_grad_(True)
            b = view.detach().float().contiguous().requires_grad_(True)
            la, lb = fn(a, tt, **kw), fn(b, tt, **kw)
            la.backward()
            lb.backward()
            assert la.dtype == torch.float32 and torch.equal(la, lb)
            assert a.grad.dtype == a.dtype and torch.equal(a.grad.float(), b.grad.to(a.dtype).float())


def test_modules_and_offset_buffers():
    name = "ohem_ignore"
    case = HC.CASES[name]
    x, t = HC.inputs(name)
    kw = HC.arguments(case)
    xt, tt = torch.from_numpy(x.copy()).to(DEV), torch.from_numpy(t.copy()).to(DEV)
    assert torch.equal(losses.OhemCrossEntropyLoss(**kw)(xt, tt), losses.ohem_cross_entropy(xt, tt, **kw))
    # logits one element off 16-byte alignment with S % 4 == 0: the peeled kernels, the same bits as the aligned 16-byte ones
    x4, t4 = HC.inputs("c16_wide")
    kw = HC.arguments(HC.CASES["c16_wide"])
    buf = torch.zeros(x4.size + 1, device=DEV)
    off = buf[1:].view(x4.shape)
    off.copy_(torch.from_numpy(x4.copy()))
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    a, b = off.requires_grad_(True), torch.from_numpy(x4.copy()).to(DEV).requires_grad_(True)
    la, lb = losses.topk_cross_entropy(a, torch.from_numpy(t4.copy()).to(DEV), **kw), losses.topk_cross_entropy(b, torch.from_numpy(t4.copy()).to(DEV), **kw)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
