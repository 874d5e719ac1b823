"""CPU half of the sweep of csrc/ptb_ensemble.hip and csrc/ptb_stack.hip (tests/test_ensemble_sweep_gpu.py is the other half):

* the float64 operator model of oracle/ensembling_oracle.py reproduces what the unmodified reference wrote into ensembling.npz and tta3.npz;
* every case of tests/ensemble_cases.py is conditioned well enough for its tolerance: the reference's own float32 chain (torch float32
  on the CPU) stays within a quarter of it -- a case that does not is tamed in its inputs, the tolerance is never widened;
* the tables reach every arm of the host dispatch, every trip count of the four-plane loop and each kind of input the issue lists."""
import numpy as np
import pytest
import torch

import ensemble_cases as EC
from conftest import load_golden
from oracle import ensembling_oracle as NO

GN = load_golden("ensembling.npz")
GT3 = load_golden("tta3.npz")
QUARTER = 0.25
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nfloat32 reference chain, worst error / tolerance: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


def _note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), r)


# ------------------------------------------------------------------------------------------------- the model against the golden vectors
def _affine(x, k, b):
    """oracle/make_golden.py:_Affine in float32: (logits, aux)."""
    y = (x * np.float32(k)).astype(np.float32) + np.float32(b)
    return y, (y * np.float32(0.5)).astype(np.float32) - np.float32(0.25)


@pytest.mark.parametrize("case", GN.by_fn("ensembler"), ids=lambda c: f"{c['name']}-{c['kwargs']['kind']}-{c['kwargs']['wrap']}-{c['kwargs']['reduction']}")
def test_model_reproduces_golden_ensembler(case):
    kw, n = case["kwargs"], case["name"]
    outs = [_affine(GN[kw["input"]], k, b) for k, b in kw["coeffs"]]
    main = NO.ensemble64([o[0] for o in outs], kw["reduction"], kw["wrap"], kw["temperature"], 1)
    if kw["keys"] is None:
        np.testing.assert_allclose(main, GN[f"{n}_out"], **EC.TOL)
        return
    aux = NO.ensemble64([o[1] for o in outs], kw["reduction"])          # the wrappers activate "logits" / element 0 only
    for key in kw["keys"]:
        np.testing.assert_allclose(main if key in ("logits", 0) else aux, GN[f"{n}_out_{key}"], **EC.TOL)


@pytest.mark.parametrize("case", GT3.cases, ids=lambda c: c["name"])
def test_model_reproduces_golden_long_stacks_and_eps(case):
    """Values at the tolerance of test_long_stacks_and_eps_oracle, gradients (float64 autograd of the same chain) at the tolerance of
    test_long_stacks_and_explicit_eps_values_and_gradients."""
    kw = case["kwargs"]
    x = GT3[case["inputs"][0]]
    if case["fn"] == "deaugment_averaging":
        red, eps, dim, period = kw["reduction"], NO.DEFAULT_EPS, 0, 5
    else:
        red, eps, dim, period = {"harmonic_mean": "hmean", "logodd_mean": "logodd"}[case["fn"]], kw["eps"], kw["dim"], 3
    stack = np.ascontiguousarray(np.moveaxis(x, dim, 0))
    want = GT3[case["output"]]
    np.testing.assert_allclose(NO.reduce64(stack, red, eps), want, rtol=1e-5, atol=1e-6)
    up = (np.arange(want.size, dtype=np.float32).reshape(want.shape) % period + 1.0).astype(np.float32)
    out, grad = NO.stack_gradient64(stack, red, eps, up)
    np.testing.assert_allclose(out, want, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(np.moveaxis(grad, 0, dim), GT3[case["output"] + "_grad"], rtol=2e-4, atol=1e-5)


def test_clamp_bounds_are_the_float32_ones():
    lo, hi = NO.clamp_bounds(1e-6)
    assert lo == float(np.float32(1e-6)) and hi == float(np.float32(1.0 - 1e-6)) and abs(hi - 0.99999899) < 1e-8
    x = np.full((1, 1), 1.0, dtype=np.float32)
    at_f32 = NO.reduce64(x, "logodd")[0]
    q = 1.0 - 1e-6
    assert abs((1.0 - at_f32) / (1.0 - q) - 1.0) > 5e-3       # a float64 bound would move logodd at the clamp by about 1 %
    assert float(torch.tensor([1.0]).clamp(max=1.0 - 1e-6)) == hi


# ------------------------------------------------------------------------------------------------- conditioning of every case
@pytest.mark.parametrize("case", EC.ALL, ids=EC.ids)
def test_case_is_conditioned_for_its_tolerance(case):
    xs = EC.inputs(case)
    want = EC.model(case, xs)
    if case.props_only:
        # the GPU file checks properties only: they must hold for the model itself
        assert not np.isnan(want).any() and want.min() >= 0.0 and want.max() <= 1.0
        return
    r = EC.ratio(EC.reference_chain_f32(case, xs), want, **EC.TOL)
    _note(case.family + (" low precision" if case.dtype != "float32" else ""), r)
    assert r <= QUARTER, r
    if case.family == "stack":
        up = EC.grad_weights(case.shape)
        _out, grad64 = NO.stack_gradient64(xs, case.reduction, case.eps, up)
        x32 = torch.from_numpy(xs).requires_grad_(True)
        (NO.torch_chain(x32, case.reduction, case.eps) * torch.from_numpy(up)).sum().backward()
        rg = EC.ratio(x32.grad.numpy(), grad64, **EC.GRAD_TOL)
        _note("stack backward", rg)
        assert rg <= QUARTER, rg


@pytest.mark.parametrize("case", EC.ALL, ids=EC.ids)
def test_inputs_follow_the_rules(case):
    """Probabilities without an activation, no probe or draw within a float32 rounding of a clamp bound (the derivative jumps there and
    two correct evaluations may take different sides), nothing negative for gmean / log1p, bounded logits for gmean / logodd."""
    xs = np.asarray(EC.inputs(case), dtype=np.float32)
    assert xs.shape == (case.T,) + case.shape and xs.dtype == np.float32
    if case.act is None:
        assert xs.min() >= 0.0 and xs.max() <= 1.0
        if case.reduction in ("hmean", "logodd"):
            for bound in NO.clamp_bounds(case.eps):
                b = np.float32(bound)
                assert not np.any(np.abs(xs - b) <= 4 * np.spacing(b)), (case.name, bound)
        flat = xs.reshape(case.T, -1)
        probes = EC.CLAMP_PROBES + (EC.EPS_PROBES if case.eps != NO.DEFAULT_EPS else ())
        if case.dtype == "float32":
            assert np.array_equal(flat[0, :len(probes)], np.asarray(probes, dtype=np.float32))
    elif EC.bounded(case):
        assert np.abs(xs * np.float32(case.temperature)).max() <= EC.BOUNDED_LOGIT * (1 + 1e-6)
    else:
        assert xs.max() == EC.SATURATING[0] and xs.min() == EC.SATURATING[1]
    again = np.asarray(EC.inputs(case))
    assert np.array_equal(xs, again)


# ------------------------------------------------------------------------------------------------- coverage of the dispatch
def test_tables_reach_every_arm():
    reached = set()
    for case in EC.ELEMENTWISE + EC.SOFTMAX:
        reached.add(EC.ensemble_arm(case))
    for case in EC.STACK:
        if case.T > EC.VIEW_KERNEL_PLANES:       # the arms x reductions are asked for at T > 8
            reached.update((EC.stack_arm(case), EC.stack_arm(case, backward=True)))
    missing = [a for a in EC.ARMS if a not in reached]
    assert not missing, missing
    assert len(EC.ARMS) == 6 + 6 + 9 + 4 + 28
    # every stack case is in scope of ptb_stack.hip, and the short ones reach both of its arms too
    assert all(EC.stack_arm(c) != "view kernels" for c in EC.STACK)
    short = {EC.stack_arm(c) for c in EC.STACK if c.T <= EC.VIEW_KERNEL_PLANES}
    assert short == {"stack_reduce_kernel<%s>/%s" % (v, r) for v in ("vector", "scalar") for r in ("hmean", "logodd")}
    # the bracketed reasons are pure: a case reaches a fall-back arm for one reason at a time
    assert not [c.name for c in EC.ELEMENTWISE + EC.SOFTMAX if "+" in EC.ensemble_arm(c)]


def test_tables_cover_the_lists_of_the_sweep():
    trips = {EC.plane_loop(c.T) for c in EC.STACK}
    assert {t for t, _ in trips} == {0, 1, 2, 3, 4} and {r for _, r in trips} == {0, 1, 2, 3}
    vec = [c for c in EC.STACK if "vector" in EC.stack_arm(c)]
    assert {EC.plane_loop(c.T)[0] for c in vec} == {0, 1, 2, 3, 4} and {EC.plane_loop(c.T)[1] for c in vec} == {0, 1, 2, 3}
    assert {c.T for c in EC.STACK if c.eps != NO.DEFAULT_EPS} >= {2, 3, 4, 5, 8} and {c.eps for c in EC.STACK} == {1e-6, 1e-3, 0.05}
    assert {c.T for c in EC.STACK if c.eps == NO.DEFAULT_EPS} == {9, 10, 12, 13, 16, 17}
    assert {c.T for c in EC.ELEMENTWISE} == {1, 2, 3, 8, 16} and {c.T for c in EC.SOFTMAX} == {1, 2, 3, 5, 16}
    vector = [c for c in EC.SOFTMAX if EC.ensemble_arm(c).startswith("ensemble_softmax_kernel")]
    assert {EC.as_bchw(c.shape, c.act, c.dim)[1] for c in vector} >= {1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16}
    for C in (3, 7, 13):                         # every reduction once per register bucket
        assert {c.reduction for c in vector if c.shape[1] == C and c.dim == 1 and not c.props_only} == set(EC.REDUCTIONS)
    assert {c.temperature for c in EC.SOFTMAX} == {1.0, 0.5, 3.0}
    other_dim = {EC.ensemble_arm(c).split("CREG=")[1].rstrip(">") for c in vector if c.dim % len(c.shape) != 1}
    assert other_dim == {"4", "8", "16"}
    assert {c.dim for c in EC.SOFTMAX} >= {0, 1, -1} and {len(c.shape) for c in EC.SOFTMAX} == {3, 4}
    # the sweep's own shapes stay within one trip of the grid; the two capped grids get one second-trip case each
    assert all(EC.grid_trips(c) == 1 for c in EC.ALL)
    assert EC.grid_trips(EC.SECOND_TRIP_STACK) == 2 and EC.grid_trips(EC.SECOND_TRIP_SOFTMAX) == 2
    assert "vector" in EC.stack_arm(EC.SECOND_TRIP_STACK) and EC.ensemble_arm(EC.SECOND_TRIP_SOFTMAX) == "ensemble_softmax_kernel<OPK=0,CREG=4>"
    assert len({c.name for c in EC.ALL}) == len(EC.ALL)


def test_as_bchw_is_the_library_factorisation():
    from pytorch_toolbelt_amd.inference import ensembling as E

    codes = {None: E._ACT_NONE, "sigmoid": E._ACT_SIGMOID, "softmax": E._ACT_SOFTMAX}
    for case in EC.ELEMENTWISE + EC.SOFTMAX + EC.LOW_PRECISION:
        assert E._as_bchw(case.shape, codes[case.act], case.dim) == EC.as_bchw(case.shape, case.act, case.dim)
    assert E._MAX_MODELS == EC.MAX_MODELS
