"""CPU half of the sweep of csrc/ptb_losses.hip (tests/test_seg_loss_sweep_gpu.py is the other half):

* the float64 model of oracle/seg_loss_oracle.py, composed into losses, reproduces what the unmodified reference wrote into losses.npz
  and losses6.npz (losses5.npz holds Lovasz cases only: nothing of it applies) and equals oracle/losses_oracle.py on the composed
  losses of the sweep's own cases; its torch half in float64 equals its numpy half;
* the tables of tests/seg_loss_cases.py reach every kernel instance the compiler emitted for ptb_losses.hip (the ``Function Name:``
  remarks of the session's forced build), except a short explicit list with reasons -- and name no instance that does not exist;
* every case is conditioned well enough for its tolerance: the reference's own float32 chain (torch float32 on the CPU) stays within a
  quarter of it, values and gradients -- a case that does not is tamed in its inputs, the tolerance is never widened.

float32 reference chain, worst error / tolerance per family (values, gradients):
    SigmoidFocalSums 0.022, 0.072   FocalScalar 0.0069, 0.0058   RegionStats 0.009, 0.17   SoftmaxFocalSums 0.063, 0.23
    FusedSegSums 0.0097, 0.2   RegionLoss 0.011, 0.072   module 0.0061, 0.1"""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import seg_loss_cases as SC
from conftest import load_golden
from oracle import losses_oracle as LO
from oracle import seg_loss_oracle as SO

GL = load_golden("losses.npz")
GL6 = load_golden("losses6.npz")
QUARTER = 0.25
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nfloat32 reference chain, worst error / tolerance (values, gradients): "
              + ", ".join("%s %.2g, %.2g" % (k, v[0], v[1]) for k, v in sorted(WORST.items())))


def _note(family, values, grads):
    old = WORST.get(family, (0.0, 0.0))
    WORST[family] = (max(old[0], values), max(old[1], grads))


# ------------------------------------------------------------------------------------------------- the model against the golden vectors
def _bchw(a):
    a = np.asarray(a)
    return a.reshape(a.shape[0], a.shape[1], -1)


def _golden_kw(case):
    kw = dict(case["kwargs"])
    if kw.pop("class_weights", None):
        kw["class_weights"] = GL["class_weights"]
    return kw


def _focal_from_model(x, labels, dense, kw, alpha_default):
    """focal_loss_with_logits / BinaryFocalLoss composed from the model's sums and map."""
    x3 = _bchw(x)
    ign_index = kw.get("ignore_index")
    normalized = kw.get("normalized", False)
    t, ign = SO.targets(x3.shape[1], None if labels is None else labels.reshape(labels.shape[0], -1), None if dense is None else _bchw(dense), ign_index)
    L, sl, sf = SO.sigmoid_focal(x3, t, ign, kw.get("gamma", 2.0), kw.get("alpha", alpha_default), kw.get("reduced_threshold"), kw.get("class_weights"),
                                 mask_term=normalized and ign_index is not None)
    norm = max(sf, 1e-6) if normalized else 1.0
    red = kw.get("reduction", "mean")
    if red == "mean":
        return sl / norm / x3.size
    if red == "sum":
        return sl / norm
    L = (L / norm).reshape(np.shape(x))
    return L.sum(axis=0) if red == "batchwise_mean" else L


@pytest.mark.parametrize("case", [c for c in GL.by_fn("focal_loss_with_logits", "binary_focal_loss") if c["kwargs"].get("activation", "sigmoid") == "sigmoid"],
                         ids=lambda c: c["name"])
def test_model_reproduces_golden_sigmoid_focal(case):
    kw = _golden_kw(case)
    x, y = GL[case["inputs"][0]], GL[case["inputs"][1]]
    labels, dense = (y, None) if y.ndim + 1 == x.ndim else (None, y)
    got = _focal_from_model(x, labels, dense, kw, 0.25 if case["fn"] == "focal_loss_with_logits" else None)
    np.testing.assert_allclose(got, GL[case["output"]], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("case", GL.by_fn("softmax_focal_loss_with_logits"), ids=lambda c: c["name"])
def test_model_reproduces_golden_softmax_focal(case):
    kw = _golden_kw(case)
    x, y = GL[case["inputs"][0]], GL[case["inputs"][1]]
    pix, sl, sf = SO.softmax_focal(_bchw(x), y.reshape(y.shape[0], -1), kw.get("class_weights"), kw.get("gamma", 2.0), kw.get("reduced_threshold"),
                                   kw.get("ignore_index", -100))
    norm = max(sf, 1e-6) if kw.get("normalized") else 1.0
    red = kw.get("reduction", "mean")
    pix = (pix / norm).reshape(y.shape)
    got = sl / norm / y.size if red == "mean" else (sl / norm if red == "sum" else (pix.sum(axis=0) if red == "batchwise_mean" else pix))
    np.testing.assert_allclose(got, GL[case["output"]], rtol=1e-5, atol=1e-5)


def _region_tensors(x, y, mode, from_logits):
    """(x [B, C, HW], labels | None, dense | None, prob) the way losses/_region.py hands a region loss to the kernels."""
    bs = x.shape[0]
    if mode == "multiclass":
        return _bchw(x), y.reshape(bs, -1), None, SO.PROB_SOFTMAX if from_logits else SO.PROB_IDENTITY
    C = 1 if mode == "binary" else x.shape[1]
    return x.reshape(bs, C, -1), None, y.reshape(bs, C, -1), SO.PROB_SIGMOID if from_logits else SO.PROB_IDENTITY


@pytest.mark.parametrize("case", GL.by_fn("dice_loss", "jaccard_loss"), ids=lambda c: c["name"])
def test_model_reproduces_golden_region_losses(case):
    kw = dict(case["kwargs"])
    x3, labels, dense, prob = _region_tensors(GL[case["inputs"][0]], GL[case["inputs"][1]], kw["mode"], kw.get("from_logits", True))
    C = x3.shape[1]
    t, ign = SO.targets(C, labels, dense, kw.get("ignore_index"))
    I, P, T = SO.region_stats(x3, t, ign, prob)
    mask = None
    if "classes" in kw:
        mask = np.zeros(C, dtype=np.uint8)
        mask[kw["classes"]] = 1
    dice = case["fn"] == "dice_loss"
    loss, _coef = SO.region_epilogue(0.0, I, P, T, 0.0, 1.0 if dice else 0.0, 0.0 if dice else 1.0, kw.get("smooth", 0.0), 1e-7, kw.get("log_loss", False),
                                     mask, len(kw["classes"]) if "classes" in kw else None)
    np.testing.assert_allclose(loss, GL[case["output"]], rtol=1e-5, atol=1e-5)


def _assert_golden_gradient(got, want):
    """The bounds of tests/test_losses_gpu.py::test_golden_gradients."""
    assert np.abs(got - want).max() <= 1e-5
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("case", GL.by_fn("grad_binary_focal", "grad_softmax_focal", "grad_dice", "grad_jaccard"), ids=lambda c: c["name"])
def test_chain_reproduces_golden_gradients(case):
    """float64 autograd of the torch half against the reference's own (float32) autograd result."""
    kw = dict(case["kwargs"])
    x, y = GL[case["inputs"][0]], GL[case["inputs"][1]]
    xt = torch.from_numpy(_bchw(x)).double().requires_grad_(True)
    if case["fn"] == "grad_softmax_focal":
        pix, _f = SO.torch_softmax_focal(xt, torch.from_numpy(y.reshape(y.shape[0], -1)), None, kw.get("gamma", 2.0), kw.get("reduced_threshold"), kw.get("ignore_index", -100))
        loss = pix.sum() / y.size
    elif case["fn"] == "grad_binary_focal":
        norm = kw.get("normalized", False)
        t, ign = SO.torch_targets(x.shape[1], y.reshape(y.shape[0], -1), None, kw.get("ignore_index"), torch.float64)
        L, F = SO.torch_sigmoid_focal(xt, t, ign, kw.get("gamma", 2.0), kw.get("alpha"), kw.get("reduced_threshold"), None, mask_term=norm)
        loss = (L.sum() / F.sum().clamp_min(1e-6) if norm else L.sum()) / x.size
    else:
        _x3, labels, dense, prob = _region_tensors(x, y, kw["mode"], True)
        t, ign = SO.torch_targets(x.shape[1], labels, dense, None, torch.float64)
        dice = case["fn"] == "grad_dice"
        loss = SO.torch_region_epilogue(None, SO.torch_region_stats(xt, t, ign, prob), 0.0, 1.0 if dice else 0.0, 0.0 if dice else 1.0, kw.get("smooth", 0.0), 1e-7,
                                        kw.get("log_loss", False))
    loss.backward()
    _assert_golden_gradient(xt.grad.numpy().reshape(x.shape), GL[case["output"]])


@pytest.mark.parametrize("case", GL6.cases, ids=lambda c: c["name"])
def test_model_reproduces_golden_fractional_gamma_with_ignore(case):
    """losses6.npz, value and gradient at the bounds of test_binary_focal_fractional_gamma_with_ignore_index: the reference's gradient
    is NaN on the ignored entries whose base 1 - pt is negative, the chain's is 0 there like the kernels'."""
    kw = dict(case["kwargs"])
    x, y = GL6[case["inputs"][0]], GL6[case["inputs"][1]]
    np.testing.assert_allclose(_focal_from_model(x, y, None, kw, None), GL6[case["output"]], rtol=1e-5, atol=1e-5)
    norm = kw.get("normalized", False)
    xt = torch.from_numpy(_bchw(x)).double().requires_grad_(True)
    t, ign = SO.torch_targets(x.shape[1], y.reshape(y.shape[0], -1), None, kw["ignore_index"], torch.float64)
    L, F = SO.torch_sigmoid_focal(xt, t, ign, kw.get("gamma", 2.0), kw.get("alpha"), kw.get("reduced_threshold"), None, mask_term=norm)
    loss = L.sum() / F.sum().clamp_min(1e-6) if norm else L.sum()
    (loss / x.size if kw.get("reduction", "mean") == "mean" else loss).backward()
    got, want = xt.grad.numpy().reshape(x.shape), GL6[case["output"] + "_grad"]
    bad = np.isnan(want)
    ignored = np.broadcast_to((y == kw["ignore_index"])[:, None], want.shape)
    assert int(bad.sum()) == case["nan_grads"] and not (bad & ~ignored).any() and (got[ignored] == 0).all()
    np.testing.assert_allclose(got[~bad], want[~bad], rtol=2e-4, atol=2e-6 * max(1.0, np.abs(want[~bad]).max()))


# ------------------------------------------------------------------------------------------------- the model against losses_oracle.py
def _oracle_targets(case, inp):
    """The target as the reference's functions take it: label maps, or dense maps with the ignore value in place."""
    return inp["labels"] if case.target == "labels" else inp["dense"]


COMPOSED = [c for c in SC.FUNCTIONS if c.family in ("SigmoidFocalSums", "SoftmaxFocalSums", "RegionLoss") and max(c.HW, c.C) <= 1024
            and not (c.family == "RegionLoss" and c.target == "labels" and c.prob == SC.PROB_SIGMOID)][::3]


@pytest.mark.parametrize("case", COMPOSED + SC.MODULES, ids=SC.ids)
def test_model_equals_losses_oracle_on_composed_losses(case):
    inp = SC.inputs(case)
    m = SC.model(case, inp)
    x, y = inp["x"], _oracle_targets(case, inp)
    if case.family == "module":
        # (module_model IS the composition of losses_oracle.py: here the sums model, composed by hand, must agree with it)
        r = SC.routed(case)
        m2 = SC.model(r, inp)
        cls, kw = case.module
        if r.family == "SoftmaxFocalSums":
            got = m2["focal"][0] / (case.B * case.HW)
        elif r.family == "SigmoidFocalSums":
            got = m2["focal"][0] / (max(m2["focal"][1], 1e-6) if kw.get("normalized") else 1.0) / SC.numel(case)
        elif r.family == "FocalScalar":
            got = m2["loss"]
        else:
            got = m2["loss"] if not r.epi.with_focal else None
        if got is not None:
            np.testing.assert_allclose(got, m["loss"], rtol=1e-9, atol=1e-12)
        return
    fkw = dict(gamma=case.gamma, alpha=case.alpha, reduced_threshold=case.threshold, ignore_index=case.ignore, class_weights=inp["cw"])
    if case.family == "SigmoidFocalSums":
        want = LO.binary_focal_loss(x, y, reduction="none", **fkw)
        np.testing.assert_allclose(m["focal"][0], np.nansum(want), rtol=1e-9)
        if case.elem:
            np.testing.assert_allclose(m["elem"], want, rtol=1e-9, atol=1e-300)
    elif case.family == "SoftmaxFocalSums":
        want = LO.softmax_focal_loss_with_logits(x, y, inp["cw"], case.gamma, "none", False, case.threshold, ignore_index=case.ignore)
        np.testing.assert_allclose(m["focal"][0], want.sum(), rtol=1e-9)
        norm = LO.softmax_focal_loss_with_logits(x, y, inp["cw"], case.gamma, "sum", True, case.threshold, ignore_index=case.ignore)
        np.testing.assert_allclose(m["focal"][0] / max(m["focal"][1], 1e-6), norm, rtol=1e-9)
    else:
        e = case.epi
        mode = "multiclass" if case.target == "labels" else "multilabel"
        rkw = dict(mode=mode, classes=e.classes, log_loss=e.log_loss, from_logits=case.prob != SC.PROB_IDENTITY, smooth=e.smooth, ignore_index=case.ignore, eps=e.eps)
        want = e.dice_weight * LO._region_loss(LO.soft_dice_score, x, y, **rkw) + e.jaccard_weight * LO._region_loss(LO.soft_jaccard_score, x, y, **rkw)
        if e.with_focal:
            fkw.pop("class_weights")
            want = want + LO.binary_focal_loss(x, y, class_weights=inp["cw"], **fkw)
        np.testing.assert_allclose(m["loss"], want, rtol=1e-9, atol=1e-12)


def test_epilogue_coefficients_are_the_derivatives_of_the_loss():
    """The closed-form coefficients of the numpy epilogue against float64 autograd of the torch one, with every option of the tail."""
    rng = np.random.default_rng(3)
    for epi in {c.epi for c in SC.REGION_LOSS}:
        C = 6
        I, P = rng.random(C) * 50, rng.random(C) * 100 + 50
        T = np.array([40.0, 0.0, 3.0, 77.0, 1.0, 0.0])
        mask = None
        if epi.classes is not None:
            mask = np.zeros(C, dtype=np.uint8)
            mask[list(epi.classes)] = 1
        kw = dict(focal_scale=0.125 if epi.with_focal else 0.0, dice_weight=epi.dice_weight, jaccard_weight=epi.jaccard_weight, smooth=epi.smooth, eps=epi.eps,
                  log_loss=epi.log_loss, class_mask=mask, n_selected=None if mask is None else int(mask.sum()))
        loss, coef = SO.region_epilogue(12.5, I, P, T, **kw)
        f = torch.tensor(12.5, dtype=torch.float64, requires_grad=True)
        s = torch.from_numpy(np.stack([I, P, T])).requires_grad_(True)
        tl = SO.torch_region_epilogue(f, s, **kw)
        tl.backward()
        np.testing.assert_allclose(loss, float(tl), rtol=1e-12)
        np.testing.assert_allclose(coef[0], 0.0 if f.grad is None else float(f.grad), rtol=1e-12)
        np.testing.assert_allclose(coef[2:], s.grad.numpy()[:2].reshape(-1), rtol=1e-10, atol=1e-15)


# ------------------------------------------------------------------------------------------------- conditioning of every case
@pytest.mark.parametrize("case", SC.ALL, ids=SC.ids)
def test_case_is_conditioned_for_its_tolerance(case):
    inp = SC.inputs(case)
    up = SC.upstream(case, inp)
    want = SC.model(case, inp)
    out64, grad64 = SC.chain_gradient(case, torch.float64, inp, up)
    for k, v in out64.items():                       # the torch half in float64 is the numpy half
        np.testing.assert_allclose(v, want[k], rtol=1e-9, atol=1e-11, err_msg=k)
    assert np.isfinite(grad64).all()
    out32, grad32 = SC.chain_gradient(case, torch.float32, inp, up)
    rv = max(SC.value_ratios(case._replace(target="soft"), out32, {k: want[k] for k in out32}).values())      # (T_c at the tolerance here: float32 sums are no counts)
    rg = SC.gradient_ratio(grad32, grad64, inp["x"])
    _note(case.family, rv, rg)
    assert rv <= QUARTER and rg <= QUARTER, (rv, rg)


@pytest.mark.parametrize("case", SC.ALL, ids=SC.ids)
def test_inputs_follow_the_rules(case):
    inp = SC.inputs(case)
    again = SC.inputs(case)
    assert all((inp[k] is None and again[k] is None) or np.array_equal(inp[k], again[k]) for k in inp)
    B, C, HW = case.B, case.C, case.HW
    assert inp["x"].shape == (B, C, HW) and inp["x"].dtype == np.float32
    assert B * HW <= 70000 and C <= 33
    ext = SC.extreme_pixels(inp["x"])[:, 0]
    assert int(ext.sum()) == SC.n_extreme(case) and ext.sum() * 8 <= B * HW
    if case.extreme:
        x, lab = inp["x"], inp["labels"]
        assert ext.any() and not ext.all() and (B == 1 or not ext[B - 1].any())    # tame and extreme pixels, with a second image one wholly tame
        m = x.max(axis=1)
        assert (m[ext] > 60).any() and (m[ext] < -60).any()                          # per-pixel maxima beyond +- 60
        below = (x - m[:, None]) <= -80
        assert below.any()                                                           # a logit 80 or more below the maximum ...
        if not case.ignored:
            assert np.take_along_axis(below, np.clip(lab, 0, C - 1)[:, None], 1)[:, 0][ext].any()     # ... that carries the pixel's label
    if case.target == "labels":
        lab = inp["labels"]
        assert lab.shape == (B, HW) and lab.dtype == np.int64
        ign = lab == case.ignore if case.ignore is not None else np.zeros(lab.shape, dtype=bool)
        assert ign.any() == bool(case.ignored) and ((lab >= 0) & (lab < C))[~ign].all()
        if case.ignored:
            first = ign[0, :min(HW, 64)]
            assert first.any() and (not first.all() or HW < 22)                      # the ignore label inside a wave ...
            if B >= 2 or HW >= 512:
                assert ign.reshape(-1)[(B - 1) * HW + (0 if B >= 2 else 256):][:min(HW, 256)].all()       # ... and a wholly ignored wave
        if case.labels == "absent" and C >= 2 and not case.extreme:
            assert not (lab == C - 1).any()
        if case.labels == "one" and not case.extreme:
            assert (lab[~ign] == C // 2).all()
    else:
        d = inp["dense"]
        assert d.shape == (B, C, HW) and d.dtype == np.float32
        ign = d == case.ignore if case.ignore is not None else np.zeros(d.shape, dtype=bool)
        assert ign.any() == bool(case.ignored) and d[~ign].min() >= 0.0 and d[~ign].max() <= 1.0
        if case.target == "dense":
            assert np.isin(d[~ign], (0.0, 1.0)).all()


# ------------------------------------------------------------------------------------------------- coverage of the dispatch
def demangle(name):
    """ptb kernel instance as the tables spell it, from the compiler's mangled name: ``name<16,false,...>`` (integers and bools only)."""
    m = re.match(r"_ZN3ptb(\d+)", name)
    assert m, name
    n = int(m.group(1))
    ident, rest = name[m.end():m.end() + n], name[m.end() + n:]
    if not rest.startswith("I"):
        return ident
    args, rest = [], rest[1:]
    while not rest.startswith("E"):
        a = re.match(r"L([ib])(n?\d+)E", rest)
        assert a, name
        args.append(("true" if a.group(2) == "1" else "false") if a.group(1) == "b" else a.group(2).replace("n", "-"))
        rest = rest[a.end():]
    return "%s<%s>" % (ident, ",".join(args))


def compiled_kernels(remarks_path):
    """Every kernel of a translation unit, from the ``Function Name:`` remarks of its kernel-resource report (read the way
    tests/test_kernel_resources.py reads them)."""
    return sorted({demangle(m.group(1)) for m in re.finditer(r"Function Name: (\S+)", open(remarks_path).read())})


def reached_arms(cases=None):
    """{kernel instance: [names of the cases that reach it]} over forward and backward of every case."""
    reached = {}
    for case in SC.ALL if cases is None else cases:
        for arm in (SC.forward_arm(case) + "+" + SC.backward_arm(case)).split("+"):
            if arm != "unsupported":
                reached.setdefault(arm, []).append(case.name)
    return reached


def test_tables_reach_every_compiled_kernel(forced_build):
    compiled = compiled_kernels(Path(forced_build["remarks_dir"]) / "ptb_losses.hip.txt")
    assert len(compiled) > 100 and "region_epilogue_kernel" in compiled and "seg_focal_pk_kernel<16,false,true,true,true>" in compiled, compiled[:5]
    reached = reached_arms()
    ghosts = sorted(set(reached) - set(compiled))
    assert not ghosts, "the restated dispatch names instances the compiler did not emit: %s" % ghosts
    missing = sorted(set(compiled) - set(reached) - set(SC.UNREACHED))
    assert not missing, "neither reached by a case nor listed in UNREACHED: %s" % missing
    stale = sorted(k for k in SC.UNREACHED if k in reached or k not in compiled)
    assert not stale, "listed in UNREACHED but reached (or not compiled): %s" % stale
    assert all(len(reason) > 20 for reason in SC.UNREACHED.values()) and len(SC.UNREACHED) <= 8


def test_tables_cover_the_lists_of_the_sweep():
    F = SC.FUNCTIONS
    assert {c.HW for c in F} >= {4, 60, 64, 128, 252, 256, 260, 250, 384, 1024, 1028, 1280, 2048}
    assert {c.B for c in F} == {1, 2, 3} and {c.C for c in F} >= {1, 2, 3, 4, 5, 8, 9, 16, 17, 19, 33}
    assert len({c.name for c in SC.ALL}) == len(SC.ALL)
    by_family = {fam: [c for c in SC.ALL if c.family == fam] for fam in SC.FAMILIES}
    assert all(by_family.values())
    assert {c.module[0] for c in SC.MODULES} == {"BinaryFocalLoss", "CrossEntropyFocalLoss", "DiceLoss", "JaccardLoss", "FocalDiceJaccardLoss"}
    for fam in SC.FAMILIES[:6]:
        cases = by_family[fam]
        # tunable 4 at 1 and at 3 on an aligned and on an unaligned shape: several trips, and an uneven last trip among them
        for t4 in (1, 3):
            capped = [c for c in cases if c.tun[1] == t4 and SC.forward_arm(c) != "unsupported"]
            assert {SC.vec_ok(c) for c in capped} >= ({True, False} if fam != "FocalScalar" else {True}), (fam, t4)
            assert all(SC.forward_trips(c)[0] >= 2 for c in capped) and any(SC.forward_trips(c)[1] for c in capped), (fam, t4)
        assert {c.tun[0] for c in cases} == {0, 1} or fam == "FocalScalar"
        # an offset of one element on each tensor, separately, on shapes that would otherwise take a vector arm
        offs = {c.off for c in cases if any(c.off)}
        assert (1, 0, 0) in offs and all(c.HW % 4 == 0 for c in cases if any(c.off)), fam
    assert {c.off for c in F} >= {(1, 0, 0), (0, 1, 1), (0, 1, 0)}
    assert any(c.off[1] and c.target == "labels" for c in F) and any(c.off[2] and c.target != "labels" for c in F)
    assert {c.tun[4] for c in F} == {0, 1} and {c.tun[3] for c in by_family["FusedSegSums"]} == {0, 1} and {c.tun[2] for c in by_family["SoftmaxFocalSums"]} == {0, 2, 4}
    # the packed kernel with tunable 20 on and off without the help of an ignore label; the slots wrap (more than 64 workgroups)
    assert any(c.tun[4] == 0 and c.ignore is None and c.family == "RegionStats" for c in F)
    wrap = [c for c in F if SC.forward_arm(c) != "unsupported" and SC.forward_grid(c)[1] > SC.SUM_SLOTS]
    assert wrap and all(c.B * c.HW // 128 > 256 for c in wrap) and {c.family for c in wrap} >= {"FocalScalar", "RegionLoss"}
    # options crossed with the arms: each occurs on several forward arms
    for name, pick in (("gamma 0", lambda c: c.gamma == 0.0 and SC.what_of(c) & 1), ("gamma 1.5", lambda c: c.gamma == 1.5), ("alpha", lambda c: c.alpha is not None),
                       ("threshold", lambda c: c.threshold is not None), ("class weights", lambda c: c.cw), ("ignore 255", lambda c: c.ignore == 255 and c.target == "labels"),
                       ("ignore 255.0", lambda c: c.ignore == 255.0 and c.target != "labels"), ("ignore -100", lambda c: c.ignore == -100.0 and c.target != "labels"),
                       ("element-wise", lambda c: c.elem), ("no term", lambda c: c.no_term), ("sigmoid", lambda c: c.prob == SC.PROB_SIGMOID),
                       ("identity", lambda c: c.prob == SC.PROB_IDENTITY)):
        arms = {SC.forward_arm(c) for c in F if c.family != "SoftmaxFocalSums" and c.family != "FocalScalar" and pick(c)}
        assert len(arms) >= 3, (name, arms)
    assert {(c.epi.log_loss, c.epi.smooth > 0, c.epi.classes is not None, c.one_launch) for c in by_family["RegionLoss"]} >= {
        (l, s, m, o) for l, s, m in ((False, False, False), (True, True, False), (True, True, True), (False, False, True)) for o in (True, False)}
    assert {c.labels for c in F} == {"rand", "absent", "one"}
    # each softmax / shared-exponent arm holds tame and extreme pixels once
    ext = {arm for c in F if c.extreme for arm in (SC.forward_arm(c) + "+" + SC.backward_arm(c)).split("+")}
    for prefix in ("seg_focal_pk_kernel", "softmax_focal_lean_kernel", "seg_fused_bwd_lean_kernel", "seg_fused_bwd_shared_kernel", "softmax_focal_kernel<4,16,0",
                   "softmax_focal_kernel<4,16,1", "softmax_focal_kernel<4,0", "softmax_focal_bwd_kernel<2", "softmax_focal_bwd_kernel<4",
                   "seg_loss_fwd_reg_kernel<4,16,3,false,true,true,true>", "seg_loss_fwd_reg_kernel<4,16,3,false,true,true,false>",
                   "seg_loss_fwd_reg_kernel<4,16,3,false,false,true,false>"):
        assert any(a.startswith(prefix) for a in ext), prefix
    # one bad-label case per forward arm that reads labels
    assert {SC.forward_arm(c) for c in SC.bad_label_cases()} == {SC.forward_arm(c) for c in F if c.target == "labels"} - {"unsupported"}


def test_restated_flags_are_the_library_constants():
    from pytorch_toolbelt_amd.losses import _kernels as K

    for name in ("SEG_FOCAL", "SEG_STATS", "SEG_HAS_IGNORE", "SEG_HAS_ALPHA", "SEG_REDUCED", "SEG_MASK_FOCAL_TERM", "SEG_ELEMWISE", "SEG_NO_TERM", "PROB_SOFTMAX",
                 "PROB_SIGMOID", "PROB_IDENTITY", "SUM_SLOTS"):
        assert getattr(K, name) == getattr(SC, name), name
