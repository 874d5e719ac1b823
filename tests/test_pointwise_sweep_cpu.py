"""CPU half of the sweep of csrc/ptb_pointwise.hip (tests/test_pointwise_sweep_gpu.py is the other half):

* the per-element float64 model of oracle/pointwise_oracle.py, composed into losses, reproduces what the unmodified reference wrote into
  losses2.npz and losses3.npz -- values and gradients, at the tolerances with which tests/test_losses2_gpu.py compares the kernels to the
  same vectors (focal_cosine of losses3.npz is no kernel of this file: nothing of it applies);
* the tables of tests/pointwise_cases.py reach every kernel instance the compiler emitted for ptb_pointwise.hip (the ``Function Name:``
  remarks of the session's forced build), except a short explicit list with reasons -- and name no instance that does not exist;
* every case is conditioned well enough for its tolerance: the reference's own float32 chain (torch float32 on the CPU) stays within a
  quarter of it, values and gradients -- a case that does not is tamed in its inputs, the tolerance is never widened; the model's analytic
  gradient is float64 autograd of the same chain;
* for t2 < 1 the bisection's knife edges (smallest |mass - 1| below 1e-4) are left out of the comparisons, and at most 1 % of a case's
  pixels or rows may be; nothing else is left out.
The per-case checks run one family of cases per test (``pointwise_cases.each`` names every case that fails).

float32 reference chain, worst error / tolerance per family (values, gradients; torch's float32 sums move the last digit from run to run):
    soft_bce 0.062, 0.087   balanced_bce 0.0068, 0.0049   qfl 0.024, 0.055   wing 0.028, 0.0095   logcosh 0.017, 0.037   soft_f1 0.0073, 0.02
    BalancedElementwise 0.0064, 0.0046   SoftCESums 0.018, 0.063   BiTemperedBinarySums 0.046, 0.032   BiTemperedRows 0.043, 0.091
    module 0.0095, 0.043"""
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import pointwise_cases as PC
from conftest import load_golden
from oracle import pointwise_oracle as PO
from test_seg_loss_sweep_cpu import compiled_kernels

GL2 = load_golden("losses2.npz")
GL3 = load_golden("losses3.npz")
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
def _reduced(elem_sum, elem, n, reduction):
    """(value, g_sum, g_elem) of a reduction over a per-element loss: the value and the upstream gradients of ``value.sum()``."""
    if reduction == "mean":
        return elem_sum / n, 1.0 / n, None
    if reduction == "sum":
        return elem_sum, 1.0, None
    return elem, 0.0, np.ones(n)


def _golden_pointwise(case):
    """(value, gradient) of a losses2.npz case from the per-element model."""
    fn, kw = case["fn"], dict(case["kwargs"])
    x, t = GL2[case["inputs"][0]], GL2[case["inputs"][1]]
    n, red = x.size, kw.get("reduction", "mean")
    if fn == "soft_bce":
        C, HW = x.shape[1], int(np.prod(x.shape[2:]))
        vec = {"chan": lambda name: GL2[name], "scalar": lambda name: np.full(C, 1.7), None: lambda name: None}
        w, pw = vec[kw.get("weight")]("wvec"), vec[kw.get("pos_weight")]("pwvec")
        ign, sf = kw.get("ignore_index", -100), kw.get("smooth_factor")
        flags = (PC.F_IGNORE if ign is not None else 0) | (PC.F_SMOOTH if sf is not None else 0)
        args = (PC.SOFT_BCE, x, t, flags, sf or 0.0, 0.0, 0.0, ign or 0.0, w, pw, C, HW)
        r = PO.pointwise(*args)
        val, g0, ge = _reduced(r["sums"][0], r["elem"], n, red)
        return val, PO.pointwise(*args, g=(g0, 0.0), g_elem=ge)["grad"]
    if fn == "balanced_bce":
        ign, gamma = kw.get("ignore_index"), np.float32(kw.get("gamma", 1.0))
        flags = PC.F_IGNORE if ign is not None else 0
        r = PO.pointwise(PC.BALANCED_BCE, x, t, flags, ignore_value=ign or 0.0)
        n_pos, n_neg = np.float32(r["sums"][2]), np.float32(r["sums"][3])
        pos = (n_neg / (n_pos + n_neg + np.float32(1e-7))) ** gamma                        # balanced_bce.py:30-34, float32 like the reference
        w = np.array([pos ** gamma, (np.float32(1.0) - pos) ** gamma], dtype=np.float64)
        if red in ("mean", "sum"):
            k = 1.0 / n if red == "mean" else 1.0
            val = -(w[0] * r["sums"][0] + w[1] * r["sums"][1]) * k
            return val, PO.pointwise(PC.BALANCED_BCE, x, t, flags, ignore_value=ign or 0.0, g=(-w[0] * k, -w[1] * k))["grad"]
        r = PO.balanced_elementwise(x, t, w, flags, ign or 0.0)
        return r["elem"], r["grad"]
    if fn == "qfl":
        beta = kw.get("beta", 2.0)
        r = PO.pointwise(PC.QFL, x, t, p0=beta)
        if red == "normalized":
            s0, s1 = r["sums"][:2]
            return s0 / s1, PO.pointwise(PC.QFL, x, t, p0=beta, g=(1.0 / s1, -s0 / s1 ** 2))["grad"]
        val, g0, ge = _reduced(r["sums"][0], r["elem"], n, red)
        return val, PO.pointwise(PC.QFL, x, t, p0=beta, g=(g0, 0.0), g_elem=ge)["grad"]
    if fn in ("wing", "logcosh"):
        width, curv = float(kw.get("width", 5)), float(kw.get("curvature", 0.5))
        args = (PC.WING, x, t, 0, width, curv, width - width * math.log(1 + width / curv)) if fn == "wing" else (PC.LOGCOSH, x, t)
        r = PO.pointwise(*args)
        val, g0, ge = _reduced(r["sums"][0], r["elem"], n, red)
        return val, PO.pointwise(*args, g=(g0, 0.0), g_elem=ge)["grad"]
    assert fn == "soft_ce", fn
    x3 = x.reshape(x.shape[0], x.shape[1], -1)
    lab = t.reshape(t.shape[0], -1)
    ign, eps = kw.get("ignore_index", -100), kw.get("smooth_factor", 0.0)
    args = (x3, lab, eps, ign is not None, ign or 0)
    r = PO.soft_ce_pixels(*args)
    val, g0, ge = _reduced(r["total"], r["pix"], lab.size, red)
    return val, PO.soft_ce_pixels(*args, g_total=g0, g_pix=None if ge is None else ge.reshape(lab.shape))["grad"]


def _fns(golden, *only):
    return sorted({c["fn"] for c in golden.cases if not only or c["fn"] in only})


@pytest.mark.parametrize("fn", _fns(GL2))
def test_model_reproduces_golden_pointwise_losses(fn):
    """losses2.npz, values and gradients at the bounds of tests/test_losses2_gpu.py::test_golden_values_and_gradients (every case of
    one loss in one test)."""
    cases = GL2.by_fn(fn)
    assert cases
    for case in cases:
        val, grad = _golden_pointwise(case)
        want = GL2[case["name"]]
        np.testing.assert_allclose(np.reshape(val, want.shape), want, rtol=2e-5, atol=1e-5, err_msg=case["name"])
        np.testing.assert_allclose(grad.reshape(GL2[case["inputs"][0]].shape), GL2[case["name"] + "_grad"], rtol=2e-5, atol=1e-5, err_msg=case["name"])


@pytest.mark.parametrize("fn", ["binary_bitempered", "bitempered"])
def test_model_reproduces_golden_bitempered_losses(fn):
    cases = GL3.by_fn(fn)
    assert len(cases) >= 6
    for case in cases:
        _golden_bitempered(case)


def _golden_bitempered(case):
    """losses3.npz at the bounds of test_binary_bitempered_native_matches_reference / test_bitempered_rows_native_matches_reference.  The
    reference ran its bisection in float32; an unreduced case leaves out the knife edges, a reduced one must not hold any."""
    kw = dict(case["kwargs"])
    x, t = GL3[case["inputs"][0]], GL3[case["inputs"][1]]
    red, sm = kw.get("reduction", "mean"), kw.get("smoothing", 0.0)
    if case["fn"] == "bitempered":
        y = np.eye(x.shape[1])[t]
        run = lambda ge: PO.bitempered_rows(x, y, kw["t1"], kw["t2"], sm, 5, ge)                                    # noqa: E731
        r = run(None)
        elem, n = r["loss"], x.shape[0]
    else:
        ign = kw.get("ignore_index")
        run = lambda ge: PO.bitempered_binary(x, t, kw["t1"], kw["t2"], sm, 5, ign is not None, ign or 0.0, 0.0, ge)    # noqa: E731
        r = run(None)
        elem, n = r["elem"], x.size
    keep = r["knife"] >= PC.KNIFE
    val, g0, ge = _reduced(elem.sum(), elem, n, red)
    grad = run(np.full(n, g0) if ge is None else ge)["grad"]
    want, want_grad = GL3[case["name"]], GL3[case["name"] + "_grad"]
    if red == "none":
        assert keep.mean() >= 0.9
        np.testing.assert_allclose(val[keep], want.reshape(-1)[keep], rtol=2e-5, atol=1e-5)
    else:
        assert keep.all(), "a reduced golden case sits on a knife edge of the bisection"
        np.testing.assert_allclose(val, want, rtol=2e-5, atol=1e-5)
    kg = np.broadcast_to(keep.reshape((-1,) + (1,) * (grad.ndim - 1)), grad.shape)
    np.testing.assert_allclose(grad[kg], want_grad.reshape(grad.shape)[kg], rtol=1e-4, atol=1e-5)


def test_model_reproduces_golden_soft_f1_losses():
    cases = GL3.by_fn("binary_soft_f1", "soft_f1")
    assert len(cases) == 3
    for case in cases:
        _golden_soft_f1(case)


def _golden_soft_f1(case):
    """losses3.npz at the bounds of test_soft_f1_native_matches_reference."""
    kw = dict(case["kwargs"])
    x, t = GL3[case["inputs"][0]], GL3[case["inputs"][1]]
    if case["fn"] == "soft_f1":
        val, grad = PO.soft_f1_softmax(x, t, kw.get("eps", 1e-6))
    else:
        ign = kw.get("ignore_index")
        args = (PC.SOFT_F1, x, t, PC.F_IGNORE if ign is not None else 0, kw.get("eps", 1e-6), 0.0, 0.0, ign or 0.0)
        s = PO.pointwise(*args)["sums"]
        den = s[1] + s[2] + 1e-6
        val = PO.soft_f1_from_counts(s[0], s[1], s[2])
        grad = PO.pointwise(*args, g=(-2.0 / den, 2.0 * s[0] / den ** 2))["grad"]
    np.testing.assert_allclose(val, GL3[case["name"]], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(grad.reshape(x.shape), GL3[case["name"] + "_grad"], rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------------------------------------- conditioning of every case
def _knife_share(case, m):
    keep = PC.kept(case, m)
    return keep, (0.0 if keep is None else 1.0 - float(keep.mean()))


@pytest.mark.parametrize("group", sorted(PC.GROUPS))
def test_case_is_conditioned_for_its_tolerance(group):
    PC.each(PC.GROUPS[group], _conditioned)


def _conditioned(case):
    inp, up = PC.inputs(case), PC.upstream(case)
    want = PC.model(case, inp, up)
    keep, _share = _knife_share(case, want)
    kg = None if keep is None else PC.expand_kept(case, keep)
    out64, grad64 = PC.chain_gradient(case, torch.float64, inp, up)
    r64 = PC.value_ratios(case, out64, want, keep)              # the torch half in float64 is the numpy half
    assert r64 and max(r64.values()) <= 1e-3, r64
    assert PC.ratio(grad64, want["grad"], keep=kg, rtol=1e-8, atol=1e-10) <= 1.0
    out32, grad32 = PC.chain_gradient(case, torch.float32, inp, up)
    rv = max(PC.value_ratios(case, out32, want, keep).values())
    rg = PC.ratio(grad32, want["grad"], keep=kg, **PC.grad_tol(case))
    _note(PC.family_of(case), rv, rg)
    assert rv <= QUARTER and rg <= QUARTER, (rv, rg)
    if keep is not None:                                        # what is left out is still finite where the model is
        assert np.isfinite(grad32.reshape(kg.shape)[~kg & np.isfinite(want["grad"].reshape(kg.shape))]).all()


def test_module_case_is_conditioned_for_its_tolerance():
    PC.each(PC.MODULES, _module_conditioned)


def _module_conditioned(case):
    """The reduced functions of the oracle (the value), float64 autograd of chain + tail (the gradient), and the same in float32."""
    inp, up = PC.inputs(case), PC.upstream(case)
    want = PC.module_model(case, inp)
    loss64, grad64 = PC.module_chain_gradient(case, torch.float64, inp, up)
    np.testing.assert_allclose(loss64, want, rtol=1e-6, atol=1e-9)       # (class-balance weights are float32 on both sides)
    loss32, grad32 = PC.module_chain_gradient(case, torch.float32, inp, up)
    rv, rg = PC.ratio(loss32, want, **PC.TOL), PC.ratio(grad32, grad64, **PC.grad_tol(case))
    _note("module", rv, rg)
    assert rv <= QUARTER and rg <= QUARTER, (rv, rg)


KNIFE_CASES = [c for c in PC.ALL if c.family.startswith("BiTempered") and c.t2 < 1.0]


def test_knife_edges_left_out_stay_under_the_cap():
    PC.each(KNIFE_CASES, _under_the_cap)


def _under_the_cap(case):
    m = PC.model(case)
    keep, share = _knife_share(case, m)
    rows = keep.size
    # (a case of fewer than 100 rows may leave out none at all: one row would already be more than 1 %)
    assert share <= PC.KNIFE_CAP, "%d of %d pixels / rows are knife edges" % (rows - keep.sum(), rows)
    if case.module is not None:
        assert keep.all(), "a reduced loss cannot leave anything out"


def test_only_the_bisection_leaves_elements_out():
    for case in PC.ALL:
        if not (case.family.startswith("BiTempered") and case.t2 < 1.0):
            m = PC.model(case)
            keep = PC.kept(case, m)
            assert keep is None or keep.all(), case.name
    assert len(KNIFE_CASES) >= 20 and {c.family for c in KNIFE_CASES} == {"BiTemperedBinarySums", "BiTemperedRows"}
    assert any(not PC.kept(c, PC.model(c)).all() for c in KNIFE_CASES), "no case has a knife edge: the measure is not exercised"


def test_tie_case_sits_on_an_exact_tie_of_the_bisection():
    """The one case that decides `mass < 1` against `mass <= 1`: at the second midpoint the mass is exactly 1 in float64 -- the model
    sends the bracket upwards there -- and no other step of the row comes near 1.  In float32 the bracket 4/3 is rounded: one ulp down
    (IEEE arithmetic here) the midpoint is 1 - 2^-24 and the mass just above 1, which is the same branch; rounded up (the kernel's
    exp2 / log2 on the MI355X) the midpoint and the mass are exactly 1, and only `<` agrees with the model -- the GPU file shows it."""
    (case,) = [c for c in PC.BT_ROWS if c.tag == "tie"]
    inp = PC.inputs(case)
    x = inp["x"]
    for dtype in (np.float32, np.float64):
        n = (x - x.max(axis=1, keepdims=True)).astype(dtype)
        hi = dtype(2.0) * (dtype(1.0) - dtype(1.0) / np.sqrt(dtype(9.0)))            # -log_t(1 / 9, 0.5)
        mid = (hi + hi * dtype(0.5)) * dtype(0.5)                                    # lo = hi / 2 after a first step with too much mass
        mass = (np.maximum(dtype(1.0) + dtype(0.5) * (n - mid), dtype(0.0)) ** 2).sum(axis=1)
        assert (mass >= 1.0).all() and abs(float(mid) - 1.0) < 1e-7
        if dtype is np.float64:
            assert mid == 1.0 and (mass == 1.0).all()
    m = PC.model(case, inp)
    assert (m["knife"] > 0.05).all() and np.isfinite(m["knife"]).all()
    assert (PO.bitempered_rows(x, inp["t"], case.t1, case.t2)["norm"] > 1.0).all()


# ------------------------------------------------------------------------------------------------- the inputs
def _branch_distance(case, inp):
    """(distance of every element from the nearest branch point of its kind, mask of the elements a case puts exactly on one)."""
    x, t = inp["x"].astype(np.float64), (None if inp["t"] is None else inp["t"].astype(np.float64))
    on = np.zeros(x.shape, dtype=bool)
    if case.family == "PointwiseSums" and case.kind == PC.WING:
        d = np.abs(t - x)
        on = d == case.p[0]
        return np.minimum(np.abs(d - case.p[0]), d), on
    if case.family == "PointwiseSums" and case.kind == PC.QFL:
        p = 1.0 / (1.0 + np.exp(-x))
        on = (x == 0.0) & (t == 0.5)
        return np.abs(p - t), on
    if case.family == "PointwiseSums" and case.kind == PC.SOFT_F1 and not case.flags & PC.F_SMOOTH:
        return np.abs(np.abs(x) - math.log((1 - case.p[0]) / case.p[0])), on
    return None, on


@pytest.mark.parametrize("group", sorted(PC.GROUPS) + ["module"])
def test_inputs_follow_the_rules(group):
    PC.each(PC.GROUPS[group] if group != "module" else PC.MODULES, _follows_the_rules)


def _follows_the_rules(case):
    inp, again = PC.inputs(case), PC.inputs(case)
    assert all((inp[k] is None and again[k] is None) or np.array_equal(inp[k], again[k]) for k in inp)
    assert case.tag == "tie" or not np.array_equal(inp["x"], PC.inputs(PC.other(case))["x"])
    assert inp["x"].dtype == np.float32 and inp["x"].size <= 70000 and inp["x"].size == (PC.numel(case))
    x = inp["x"]
    # extreme cases: about one element in 16 beyond 20, none beyond 80; tame cases: none beyond 20
    span = np.abs(x - inp["t"]) if (case.family == "PointwiseSums" and case.kind in (PC.WING, PC.LOGCOSH)) else np.abs(x)
    if case.extreme:
        share = float((span >= 19.9).mean())
        assert 1 / 32 <= share <= 1 / 12 and span.max() <= 80.5, (share, span.max())
    else:
        assert span.max() < 20.0
    dist, on = _branch_distance(case, inp)
    if dist is not None:
        assert (dist[~on] >= PC.EDGE).all(), dist[~on].min()
    assert on.any() == (case.tag == "on-target" or (case.family == "PointwiseSums" and case.kind == PC.WING and x.size > 2))
    if case.family.startswith("BiTempered") and case.t2 < 1.0 and case.tag != "tie":
        a = x if case.family == "BiTemperedRows" else np.stack([-x, x], axis=1)
        n = a.astype(np.float64) - a.astype(np.float64).max(axis=1, keepdims=True)
        assert (np.abs(n + 1.0 / (1.0 - case.t2)) >= PC.EDGE).all()
        base = PC.support_distance(a, case.t2)
        assert (np.abs(base) >= PC.SUPPORT_MARGIN).all()
        if a.shape[0] * a.shape[1] >= 500 and case.family == "BiTemperedRows" and a.shape[1] > 2:
            assert (base < 0).any(), "no class outside the support"
    if case.ignore is not None and case.family != "SoftCESums":
        ign = inp["t"] == case.ignore
        assert ign.any() and not ign.all()
    if case.family == "SoftCESums":
        lab = inp["labels"]
        ign = lab == case.ignore if case.ignore is not None else np.zeros(lab.shape, dtype=bool)
        assert lab.dtype == np.int64 and ((lab >= 0) & (lab < case.C))[~ign].all()
        assert ign.any() == (case.labels in ("some", "image"))
        if case.labels == "image":
            assert ign[-1].all() and not ign[0].all() or case.HW == 1
        if case.labels == "absent":
            assert not (lab == case.C - 1).any()
    if case.family == "BiTemperedRows":
        y = inp["t"]
        np.testing.assert_allclose(y.sum(axis=1), 1.0, rtol=1e-5)
        assert np.isin(y, (0.0, 1.0)).all() != case.soft or case.C == 1


# ------------------------------------------------------------------------------------------------- coverage of the dispatch
def reached_arms(cases=None):
    """{kernel instance: [names of the cases that reach it]} over forward and backward of every case."""
    reached = {}
    for case in PC.ALL if cases is None else cases:
        for arm in (PC.forward_arm(case) + "+" + PC.backward_arm(case)).split("+"):
            reached.setdefault(arm, []).append(case.name)
    return reached


def test_tables_reach_every_compiled_kernel(forced_build):
    compiled = compiled_kernels(Path(forced_build["remarks_dir"]) / "ptb_pointwise.hip.txt")
    assert len(compiled) >= 40 and "bitempered_rows_kernel<true>" in compiled and "soft_ce_kernel<4,16,1>" in compiled, compiled[:5]
    reached = reached_arms()
    ghosts = sorted(set(reached) - set(compiled))
    assert not ghosts, "the restated dispatch names instances the compiler did not emit: %s" % ghosts
    missing = sorted(set(compiled) - set(reached) - set(PC.UNREACHED))
    assert not missing, "neither reached by a case nor listed in UNREACHED: %s" % missing
    stale = sorted(k for k in PC.UNREACHED if k in reached or k not in compiled)
    assert not stale, "listed in UNREACHED but reached (or not compiled): %s" % stale
    assert all(len(reason) > 20 for reason in PC.UNREACHED.values()) and len(PC.UNREACHED) <= 4


def test_tables_cover_the_lists_of_the_sweep():
    F = PC.FUNCTIONS
    assert len({c.name for c in PC.ALL}) == len(PC.ALL)
    by = {fam: [c for c in F if c.family == fam] for fam in PC.FAMILIES}
    assert all(by.values()) and {c.kind for c in by["PointwiseSums"]} == set(range(6))
    streams = [[c for c in by["PointwiseSums"] if c.kind == k] for k in range(6)] + [by["BalancedElementwise"], by["SoftCESums"], by["BiTemperedBinarySums"]]
    for cases in streams:
        # grid-stride tails: tunable 4 at 1, group counts 1 .. 769; a second step that holds a single group among them
        capped = [c for c in cases if c.tun[1] == 1]
        assert {PC.forward_groups(c)[0] for c in capped} >= set(PC.TRIP_GROUPS), cases[0].name
        assert all(PC.forward_grid(c) == 1 for c in capped) and {PC.forward_trips(c) for c in capped} >= {(1, 1), (1, 255), (1, 0), (2, 1), (3, 1), (4, 1)}
        # slots: more than 64 workgroups, so that some slots take two atomics and others one
        grids = {PC.forward_grid(c) for c in cases}
        if cases[0].family != "BalancedElementwise":            # (the element-wise form has no sums)
            assert 65 in grids and (129 in grids or cases[0].family == "SoftCESums"), (cases[0].name, sorted(grids)[-3:])
    for cases in streams[:7]:
        assert {PC.numel(c) % 4 for c in cases} >= {0, 1, 3} and {c.tun[0] for c in cases} == {0, 1}
        vec = lambda c, b: PC.pw_vec(c, b)                                                     # noqa: E731
        assert any(vec(c, False) for c in cases) and any(not vec(c, False) for c in cases)
        offs = {c.off for c in cases if c.off}
        names = {"x", "t", "grad"} | ({"out", "grad_elem"} if any(PC.has_map(c) for c in cases) else set())
        assert offs == {((n, o),) for n in names for o in (1, 4)}, offs
        for c in cases:
            if c.off:                                                                          # offset 1 falls to the scalar arm, offset 4 stays on the vector arm
                (name, o), = c.off
                touched_fwd = name in ("x", "t") or name == "out"
                touched_bwd = name in ("x", "t", "grad", "grad_elem")
                assert vec(c, False) == (o == 4 or not touched_fwd) and vec(c, True) == (o == 4 or not touched_bwd), c.name
    sce = by["SoftCESums"]
    assert {c.C for c in sce} >= {1, 2, 4, 5, 8, 9, 16, 17, 33} and {c.HW for c in sce} >= {1, 3, 4, 8, 260} and {c.eps for c in sce} >= {0.0, 0.1, 1.0}
    assert {(c.C, c.HW) for c in sce} >= {(C, HW) for C in (1, 2, 4, 5, 8, 9, 16, 17, 33) for HW in (1, 3, 4, 8, 260)}
    assert {c.labels for c in sce} == {"rand", "some", "image", "absent"} and {c.elem for c in sce} == {True, False}
    assert {c.off for c in sce if c.off} == {((n, o),) for n in ("x", "labels", "pix_out", "grad", "grad_pix") for o in (1, 4)} | {(("x", 1),)}
    for c in sce:
        if c.off and c.elem:
            (name, o), = c.off
            assert PC.sce_vec(c, False) == (o == 4 or name in ("grad", "grad_pix")) and PC.sce_vec(c, True) == (o == 4 or name == "pix_out"), c.name
    assert {PC.forward_arm(c) for c in PC.bad_label_cases()} == {PC.forward_arm(c) for c in sce}
    pw = by["PointwiseSums"]
    assert {(c.B, c.C, c.HW) for c in pw if c.chan} >= set(PC.CHAN_SHAPES) and {c.chan for c in pw} == {"", "w", "pw", "wpw"}
    for shape in PC.CHAN_SHAPES:
        assert {(c.chan, bool(c.flags & PC.F_SMOOTH), c.ignore is not None) for c in pw if (c.B, c.C, c.HW) == shape} >= {
            (ch, s, s) for ch in ("w", "pw", "wpw") for s in (False, True)}
    assert {c.p[0] for c in pw if c.kind == PC.QFL} >= set(PC.QFL_BETAS) and {c.p[0] for c in pw if c.tag == "on-target"} >= {0.0, 0.5, 1.0, 2.0}
    assert {c.p[:2] for c in pw if c.kind == PC.WING} == set(PC.WING_PARAMS)
    f1 = [c for c in pw if c.kind == PC.SOFT_F1]
    assert {(bool(c.flags & PC.F_SMOOTH), c.ignore is not None) for c in f1} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(c.p[0] == 0.05 and c.ignore is not None for c in f1) and any(c.p[0] == 0.05 and c.ignore is None for c in f1)
    for k in range(6):                                          # every kind (and every family) has a tame and an extreme case
        assert {c.extreme for c in pw if c.kind == k} == {False, True}, k
    assert all({c.extreme for c in by[fam]} == {False, True} for fam in ("BalancedElementwise", "SoftCESums", "BiTemperedBinarySums"))
    binary, rows = by["BiTemperedBinarySums"], by["BiTemperedRows"]
    assert {(c.t1, c.t2, c.smoothing, c.ignore is not None) for c in binary} >= {(a, b, s, i) for a, b in PC.BT_TEMPS for s in (0.0, 0.1) for i in (False, True)}
    assert {(c.C, c.t1, c.t2) for c in rows} >= {(K, a, b) for K in (1, 2, 63, 64, 65, 129, 257) for a, b in PC.BT_TEMPS}
    assert {c.B for c in rows} >= {1, 3, 4, 5, 8197} and {c.soft for c in rows} == {False, True} and {c.smoothing for c in rows} == {0.0, 0.1}
    assert all(c.smoothing == 0.0 for c in rows if c.C == 1)
    assert any(PC.forward_trips(c)[0] >= 2 for c in rows) and any(PC.forward_trips(c)[0] >= 2 and c.t2 < 1 for c in rows)


def test_restated_constants_are_the_library_constants():
    from pytorch_toolbelt_amd.losses import _kernels as K
    from pytorch_toolbelt_amd.losses import _pointwise as P

    for name in ("SOFT_BCE", "BALANCED_BCE", "QFL", "WING", "LOGCOSH", "SOFT_F1", "F_IGNORE", "F_SMOOTH"):
        assert getattr(P, name) == getattr(PC, name), name
    assert K.SUM_SLOTS == PC.SUM_SLOTS
    assert (PO.PW_SOFT_BCE, PO.PW_BALANCED_BCE, PO.PW_QFL, PO.PW_WING, PO.PW_LOGCOSH, PO.PW_SOFT_F1) == tuple(range(6))


def test_slot_layout_adds_up_to_the_sums():
    """``slot_sums`` spreads the per-element contributions over the slots the workgroups add into: the slots add up to the sums, 65
    workgroups give slot 0 two of them, and fewer than 64 leave the rest empty."""
    for case in PC.FUNCTIONS:
        if case.family in ("BalancedElementwise", "BiTemperedRows") or PC.numel(case) > 20000 and case.seed % 3:
            continue
        m = PC.model(case)
        finite = np.isfinite(m["slots"]).all()
        if finite:
            np.testing.assert_allclose(m["slots"].sum(axis=0)[:m["sums"].size] if case.family == "PointwiseSums" else m["slots"].sum(axis=0)[:1],
                                       m["sums"] if case.family == "PointwiseSums" else m["slots"].sum(axis=0)[:1], rtol=1e-9, atol=1e-9)
        grid = PC.forward_grid(case)
        used = np.unique(PC.slot_of(case))
        assert used.size == min(grid, PC.SUM_SLOTS, -(-PC.forward_groups(case)[0] // 256)) and (m["slots"][[s for s in range(64) if s not in used]] == 0).all()
