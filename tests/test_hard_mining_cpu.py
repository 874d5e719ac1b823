"""CPU: the host form of the hard-example-mining losses (losses/hard_mining.py) against the float64 model of tests/hard_mining_cases.py and
against the literal torch chain, the near-cut condition on the model's cases, the argument validation of the native entry points (which
returns before any launch), the Python errors and the exports."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hard_mining_cases as HC
import seg_loss_cases as SC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd import losses
from pytorch_toolbelt_amd.losses import hard_mining as HM

MAX_UNDECIDED = 3            # per selection set, the cut element itself included


def _run(name, **extra):
    return HC.run(name, losses.topk_cross_entropy, losses.ohem_cross_entropy, **extra)


@pytest.mark.parametrize("name", list(HC.CASES))
def test_host_form_against_the_model(name):
    HC.check(name, *_run(name))


@pytest.mark.parametrize("name", HC.TIE_FREE)
def test_near_cut_condition_of_the_cases(name):
    """On the model alone: at most MAX_UNDECIDED elements of a set lie within the near-cut width of ``thr``, and no element lies that
    close to the OHEM threshold ``t0`` (where a flip would change the kept count)."""
    want = HC.model(name)
    assert want.undecided_per_set.max() <= MAX_UNDECIDED, (name, want.undecided_per_set)
    assert want.near_t0 == 0, (name, want.near_t0)
    kept = np.atleast_1d(want.kept)
    assert ((want.undecided_per_set >= 1) == (kept > 0)).all()                 # the cut element is undecided by definition


def test_the_cases_reach_what_they_claim():
    C = HC.CASES
    assert {k.S for k in C.values()} == {5, 1023, 1024, 1027, 3077, 4096, 660}
    assert {k.C for k in C.values() if k.mode == "multiclass"} >= {2, 4, 5, 8, 9, 16, 17, 19}
    assert HC.model("kone").kept == 1 and (HC.model("kone_per_sample").kept == 1).all()
    assert HC.model("k100").kept == 3 * 3077
    n = 3 * 1027
    above = HC.model("ohem_above")
    assert 100 < above.kept < n                                                 # the threshold branch
    assert HC.model("ohem_floor").kept == 700                                   # the floor
    l, valid, _ = HC._elements("ohem_equal")
    assert HC.model("ohem_equal").kept == HC.min_kept("ohem_equal") == int((l > HC.t0_of(C["ohem_equal"])).sum()) > 0
    assert HC.model("ohem_nothing").kept == 0 and np.isposinf(HC.model("ohem_nothing").thr) and HC.model("ohem_nothing").loss == 0
    assert HC.model("ohem_everything").kept == n
    assert list(HC.model("ignore_sample_per_sample").kept)[1] == 0 and list(HC.model("ignore_sample_per_sample").kept)[0] > 0
    assert HC.model("ignore_all").kept == 0 and not HC.model("ignore_all").grad.any()
    for name in ("tie_identical", "tie_identical_per_sample"):                  # every weight is kept / n
        want = HC.model(name)
        kept = np.atleast_1d(want.kept)
        w = want.weight.reshape(kept.size, -1)
        np.testing.assert_allclose(w, np.broadcast_to((kept / w.shape[1])[:, None], w.shape), rtol=1e-12)
    for name, inside in (("tie_groups_hard", "hard"), ("tie_groups_easy", "easy"), ("tie_ohem_floor", "hard")):
        w = np.unique(HC.model(name).weight)
        assert (len(w) == 2 and w[0] == 0 and 0 < w[1] < 1) if inside == "hard" else (len(w) == 2 and 0 < w[0] < 1 and w[1] == 1), (name, w)


# ---------------------------------------------------------------------------------------------------------------- the torch chain
def _element_losses(name, xt, tt):
    case = HC.CASES[name]
    if case.mode == "multiclass":
        valid = tt != HC.IGNORE
        return F.cross_entropy(xt, torch.where(valid, tt, torch.zeros_like(tt)), reduction="none")[valid]
    valid = tt != HC.IGNORE
    return F.binary_cross_entropy_with_logits(xt, torch.where(valid, tt, torch.zeros_like(tt)), reduction="none")[valid]


@pytest.mark.parametrize("name", [n for n in HC.TIE_FREE if HC.CASES[n].rule == "topk" and not HC.CASES[n].per_sample and HC.CASES[n].ignore != "all"])
def test_against_the_literal_topk_chain(name):
    x, t = HC.inputs(name)
    xt, tt = torch.from_numpy(x.copy()).requires_grad_(True), torch.from_numpy(t.copy())
    kept = int(HC.model(name).kept)
    chain = _element_losses(name, xt, tt).flatten().topk(kept)[0].mean()
    loss, thr, got_kept, grad = _run(name)
    assert int(got_kept) == kept
    np.testing.assert_allclose(loss.item(), chain.item(), rtol=SC.TOL["rtol"], atol=SC.TOL["atol"])
    (chain * float(HC.model(name).coef[0])).backward()
    # the chain's float32 losses may order two near-cut elements the other way: the elements both forms keep, and both drop, agree
    want = HC.model(name)
    bound = SC.GRAD_TOL["rtol"] * np.abs(want.grad) + SC.GRAD_TOL["atol"] * want.scale
    off = (np.abs(grad.numpy() - xt.grad.numpy()) > bound) & ~want.undecided
    assert not off.any(), (name, int(off.sum()))


@pytest.mark.parametrize("name", ("k100", "ignore"))
def test_k100_is_cross_entropy(name):
    x, t = HC.inputs(name)
    xt, tt = torch.from_numpy(x.copy()).requires_grad_(True), torch.from_numpy(t.copy())
    want = F.cross_entropy(xt, tt, ignore_index=HC.IGNORE)
    xg = torch.from_numpy(x.copy()).requires_grad_(True)
    got = losses.topk_cross_entropy(xg, tt, k=100.0, ignore_index=HC.IGNORE)
    np.testing.assert_allclose(got.item(), want.item(), rtol=SC.TOL["rtol"], atol=SC.TOL["atol"])
    want.backward()
    got.backward()
    n = int((tt != HC.IGNORE).sum())
    np.testing.assert_allclose(xg.grad.numpy(), xt.grad.numpy(), rtol=SC.GRAD_TOL["rtol"], atol=SC.GRAD_TOL["atol"] / n)


def test_modules_are_the_functions_and_half_logits_are_widened():
    for name, module in (("ignore", losses.TopKCrossEntropyLoss), ("ohem_per_sample", losses.OhemCrossEntropyLoss), ("binary_s1027", losses.TopKCrossEntropyLoss)):
        x, t = HC.inputs(name)
        kw = HC.arguments(HC.CASES[name])
        fn = losses.topk_cross_entropy if module is losses.TopKCrossEntropyLoss else losses.ohem_cross_entropy
        xt, tt = torch.from_numpy(x.copy()), torch.from_numpy(t.copy())
        assert torch.equal(module(**kw)(xt, tt), fn(xt, tt, **kw))
        assert torch.equal(module(**kw)(xt.half(), tt), fn(xt.half().float(), tt, **kw))
        assert torch.equal(module(**kw)(xt.bfloat16(), tt), fn(xt.bfloat16().float(), tt, **kw))
    assert losses.TopKCrossEntropyLoss().k == 10.0 and losses.OhemCrossEntropyLoss().min_kept == 100_000 and losses.OhemCrossEntropyLoss().thresh == 0.7


# ---------------------------------------------------------------------------------------------------------------- native validation
def test_argument_validation_without_gpu():
    """Every refusal below returns before the first launch, so the pointers are never followed: any non-null value serves."""
    lib = N.load()
    P = 1 << 20                                             # stands for a device pointer, 16-byte aligned
    B, C, S = 2, 4, 48

    def fwd(**kw):
        a = dict(logits=P, labels=P, dense=None, B=B, C=C, S=S, per_sample=0, rule=0, k=10.0, t0=0.5, min_kept=10, map=P, ws=P, ws_bytes=1 << 20, loss=P,
                 thr=P, kept=P, inv=P, select=P, flag=P)
        a.update(kw)
        return lib.ptb_hardce_fwd(a["logits"], a["labels"], a["dense"], a["B"], a["C"], a["S"], 0, 0, 0.0, a["per_sample"], a["rule"], a["k"], a["t0"],
                                  a["min_kept"], a["map"], a["ws"], a["ws_bytes"], a["loss"], a["thr"], a["kept"], a["inv"], a["select"], a["flag"], None)

    def bwd(**kw):
        a = dict(logits=P, labels=P, dense=None, map=P, B=B, C=C, S=S, per_sample=0, coef=P, select=P, grad=P)
        a.update(kw)
        return lib.ptb_hardce_bwd(a["logits"], a["labels"], a["dense"], a["map"], a["B"], a["C"], a["S"], a["per_sample"], a["coef"], a["select"],
                                  a["grad"], None)

    for kw in (dict(logits=None), dict(labels=None), dict(dense=P), dict(B=0), dict(C=0), dict(S=0), dict(map=None), dict(map=P + 2), dict(select=None),
               dict(select=P + 1)):
        assert fwd(**kw) == -1, kw
        assert bwd(**kw) == -1, kw
    for kw in (dict(rule=2), dict(rule=-1), dict(k=0.0), dict(k=100.5), dict(k=float("nan")), dict(rule=1, t0=0.0), dict(rule=1, t0=-1.0),
               dict(rule=1, t0=float("inf")), dict(rule=1, t0=float("nan")), dict(rule=1, min_kept=-1), dict(ws=None), dict(ws=P + 8), dict(loss=None),
               dict(thr=None), dict(kept=None), dict(inv=None), dict(flag=None)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(coef=None), dict(grad=None)):
        assert bwd(**kw) == -1, kw
    need = lib.ptb_hardce_workspace_bytes(0, B, C, S, 0)
    assert need == 16 + 264 * 4 and fwd(ws_bytes=need - 1) == -1                # one slot, one set's state
    assert lib.ptb_hardce_workspace_bytes(0, B, C, S, 1) == 2 * (16 + 264 * 4)
    assert lib.ptb_hardce_workspace_bytes(1, 3, 5, 4097, 0) == 16 * 16 + 264 * 4      # ceil(3 * 5 * 4097 / 4096) slots
    assert lib.ptb_hardce_workspace_bytes(1, 3, 5, 4097, 1) == 3 * (16 * 6 + 264 * 4)
    for bad in ((0, 0, C, S, 0), (0, B, 0, S, 0), (0, B, C, 0, 0)):
        assert lib.ptb_hardce_workspace_bytes(*bad) == -1, bad
    # a selection set of 2^31 or more elements
    assert lib.ptb_hardce_workspace_bytes(0, 1, C, 1 << 31, 0) == N.PTB_EUNSUPPORTED and lib.ptb_hardce_workspace_bytes(0, 1, C, (1 << 31) - 1, 0) > 0
    assert lib.ptb_hardce_workspace_bytes(0, 2, C, 1 << 30, 0) == N.PTB_EUNSUPPORTED and lib.ptb_hardce_workspace_bytes(0, 2, C, 1 << 30, 1) > 0
    assert lib.ptb_hardce_workspace_bytes(1, 1, 4, 1 << 29, 1) == N.PTB_EUNSUPPORTED and lib.ptb_hardce_workspace_bytes(0, 1, 4, 1 << 29, 1) > 0
    assert fwd(S=1 << 31) == N.PTB_EUNSUPPORTED and bwd(S=1 << 31) == N.PTB_EUNSUPPORTED
    assert fwd(B=2, S=1 << 30) == N.PTB_EUNSUPPORTED and bwd(B=2, S=1 << 30) == N.PTB_EUNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- python errors
def test_constructor_and_call_errors():
    x, t = torch.zeros(2, 3, 4, 5), torch.zeros(2, 4, 5, dtype=torch.int64)
    for cls in (losses.TopKCrossEntropyLoss, losses.OhemCrossEntropyLoss):
        with pytest.raises(ValueError, match="mode"):
            cls("panoptic")
        with pytest.raises(ValueError, match="reduction"):
            cls(reduction="sum")
        with pytest.raises(ValueError, match="per_sample"):
            cls(reduction="none")
        assert cls(per_sample=True, reduction="none")(x, t).shape == (2,)
    for k in (0.0, -1.0, 100.1, float("nan")):
        with pytest.raises(ValueError, match="percentage"):
            losses.TopKCrossEntropyLoss(k=k)
        with pytest.raises(ValueError, match="percentage"):
            losses.topk_cross_entropy(x, t, k=k)
    for thresh in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="thresh"):
            losses.OhemCrossEntropyLoss(thresh=thresh)
        with pytest.raises(ValueError, match="thresh"):
            losses.ohem_cross_entropy(x, t, thresh=thresh)
    for min_kept in (-1, 2.5):
        with pytest.raises(ValueError, match="min_kept"):
            losses.OhemCrossEntropyLoss(min_kept=min_kept)
    with pytest.raises(ValueError, match="per_sample"):
        losses.topk_cross_entropy(x, t, reduction="none")
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        losses.topk_cross_entropy(x[0], t)
    with pytest.raises(ValueError, match="integer labels"):
        losses.topk_cross_entropy(x, t.float())
    with pytest.raises(ValueError, match="integer labels"):
        losses.ohem_cross_entropy(x, t[:, :3])
    with pytest.raises(ValueError, match="does not match"):
        losses.topk_cross_entropy(x, torch.zeros(2, 3, 4, 4), "multilabel")
    with pytest.raises(ValueError, match="one channel"):
        losses.ohem_cross_entropy(x, torch.zeros(2, 3, 4, 5), "binary")
    with pytest.raises(TypeError, match="floating-point"):
        losses.topk_cross_entropy(t, t)
    with pytest.raises(RuntimeError, match="Class values must be smaller"):
        losses.topk_cross_entropy(x, t + 3)
    assert torch.isfinite(losses.topk_cross_entropy(x, t + 3, ignore_index=3))
    assert losses.topk_cross_entropy(torch.zeros(2, 3, 2, 4, 5), torch.zeros(2, 2, 4, 5, dtype=torch.int64)).shape == ()


def test_return_threshold_and_empty_sets():
    x, t = torch.randn(2, 3, 4, 5, generator=torch.Generator().manual_seed(1)), torch.full((2, 4, 5), 255, dtype=torch.int64)
    xg = x.clone().requires_grad_(True)
    loss, thr, kept = losses.ohem_cross_entropy(xg, t, ignore_index=255, per_sample=True, reduction="none", return_threshold=True)
    assert loss.tolist() == [0.0, 0.0] and torch.isposinf(thr).all() and kept.tolist() == [0, 0] and kept.dtype == torch.int64 and thr.dtype == torch.float32
    loss.sum().backward()
    assert not xg.grad.any()
    out = losses.topk_cross_entropy(x, t.clamp(max=2), return_threshold=True)
    assert len(out) == 3 and out[0].shape == out[1].shape == out[2].shape == () and int(out[2]) == 4


def test_exports():
    assert HM.__all__ == ["TopKCrossEntropyLoss", "OhemCrossEntropyLoss", "topk_cross_entropy", "ohem_cross_entropy"]
    for name in HM.__all__:
        assert getattr(losses, name) is getattr(HM, name)
    for name in ("ptb_hardce_workspace_bytes", "ptb_hardce_fwd", "ptb_hardce_bwd"):
        assert name in N.SIGNATURES and hasattr(N.load(), name)
    assert "no counterpart" in HM.__doc__
