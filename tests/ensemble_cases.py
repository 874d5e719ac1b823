"""Case tables shared by the sweeps of the reduce-over-models kernels (tests/test_ensemble_sweep_cpu.py, tests/test_ensemble_sweep_gpu.py):
csrc/ptb_ensemble.hip behind ``Ensembler`` / ``ApplySigmoidTo`` / ``ApplySoftmaxTo`` and csrc/ptb_stack.hip behind ``stack_reduce``.

A case holds the shapes, T, activation, temperature, softmax dim, reduction, eps, dtype, pointer offset (in elements) and a seed; its
inputs are a function of the case only.  ``ensemble_arm`` / ``stack_arm`` restate the host dispatch (``ptb_ensemble_reduce``,
``ptb_stack_reduce[_bwd]``, ``_as_bchw``, ``stack_reduce``, ``_ensemble_native``) in plain Python and name the kernel instance a case will
launch, so that the CPU file can assert that the tables reach every arm: coverage is a checked property of the tables."""
from collections import namedtuple

import numpy as np

from oracle import ensembling_oracle as NO

REDUCTIONS = NO.REDUCTIONS
NONLINEAR = REDUCTIONS[2:]
DEFAULT_EPS = NO.DEFAULT_EPS
MAX_MODELS = 16                     # ptb_ensemble.hip MAX_MODELS / ensembling._MAX_MODELS: longer lists take the stack path
VIEW_KERNEL_PLANES = 8              # stack_reduce: up to 8 planes with the default eps belong to the view kernels (out of scope here)
ENSEMBLE_GRID_CAP, STACK_GRID_CAP = 16384, 256 * 16     # workgroups of 256 lanes; above the cap the grid-stride loops make a second trip

TOL = dict(rtol=1e-5, atol=1e-5)            # activated and non-linear values against the float64 model (tests/test_ensembling_gpu.py TOL)
GRAD_TOL = dict(rtol=2e-4, atol=2e-5)       # gradients (the golden gradient tests)
MEAN_TOL = dict(rtol=1e-6, atol=1e-7)       # plain mean against the float32 list-order sum divided by T

Case = namedtuple("Case", "family name shape T act temperature dim reduction eps dtype offset seed scalar props_only")


def make_case(family, shape, T, reduction, act=None, temperature=1.0, dim=1, eps=DEFAULT_EPS, dtype="float32", offset=0, seed=0, scalar=0,
              props_only=False):
    shape = tuple(shape)
    name = "%s-%s-T%d-%s" % (family, "x".join(map(str, shape)), T, reduction)
    if act:
        name += "-%s%s-t%g" % (act, "" if act == "sigmoid" else "@%d" % dim, temperature)
    if eps != DEFAULT_EPS:
        name += "-eps%g" % eps
    if dtype != "float32":
        name += "-" + dtype
    if offset:
        name += "-off%d" % offset
    if scalar:
        name += "-scalar"
    if props_only:
        name += "-saturating"
    return Case(family, name, shape, T, act, float(temperature), dim, reduction, eps, dtype, offset, seed, scalar, props_only)


def numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def offset_index(case):
    """Which of the T inputs of an ensemble case starts ``case.offset`` elements into its allocation (a stack is offset as a whole)."""
    return case.T // 2


# ------------------------------------------------------------------------------------------------- the host dispatch, restated
def as_bchw(shape, act, dim):
    """ensembling._as_bchw: the (B, C, HW) factorisation handed to ptb_ensemble_reduce."""
    if act != "softmax":
        return 1, 1, numel(shape)
    d = dim % len(shape)
    return numel(shape[:d]), int(shape[d]), numel(shape[d + 1:])


def _opk(reduction):
    """with_reduction3: 0 = sum / mean, 2 = gmean, 1 = every other non-linear reduction."""
    return 0 if reduction in ("sum", "mean") else (2 if reduction == "gmean" else 1)


def _aligned16(case):
    """Every float32 allocation starts on a 16-byte boundary (the GPU file asserts it); half / bfloat16 sources are widened into a
    fresh float32 tensor first, so their offset never reaches the kernel."""
    return case.dtype != "float32" or case.offset % 4 == 0


def ensemble_arm(case):
    """The instance ptb_ensemble_reduce launches for an ``elementwise`` or ``softmax`` case; the scalar / generic arms carry the
    reason(s) in brackets: tunable (ptb_set_tunable(1, 1)), alignment, size (n % 4), HW (HW % 4), C (C > 16)."""
    assert case.family in ("elementwise", "softmax") and 1 <= case.T <= MAX_MODELS
    B, C, HW = as_bchw(case.shape, case.act, case.dim)
    why = (["tunable"] if case.scalar else []) + ([] if _aligned16(case) else ["alignment"])
    if case.act == "softmax":
        why += (["HW"] if HW % 4 else []) + (["C"] if C > 16 else [])
        if not why:
            return "ensemble_softmax_kernel<OPK=%d,CREG=%d>" % (_opk(case.reduction), 4 if C <= 4 else (8 if C <= 8 else 16))
        return "ensemble_softmax_generic_kernel[%s]" % "+".join(why)
    act = 1 if case.act == "sigmoid" else 0
    why += ["size"] if (B * C * HW) % 4 else []
    if not why:
        return "ensemble_kernel<OPK=%d,ACT=%d>" % (_opk(case.reduction), act)
    return "ensemble_scalar_kernel<ACT=%d>[%s]" % (act, "+".join(why))


def stack_arm(case, backward=False):
    """The instance ptb_stack_reduce / ptb_stack_reduce_bwd launches for a ``stack`` case called through ``stack_reduce`` (the output,
    the upstream gradient and the gradient are fresh allocations there: only the stack itself can be off the 16-byte grid)."""
    assert case.family == "stack"
    if not (case.T > VIEW_KERNEL_PLANES or (case.eps != DEFAULT_EPS and case.reduction in ("hmean", "logodd"))):
        return "view kernels"
    vector = not case.scalar and numel(case.shape) % 4 == 0 and _aligned16(case)
    return "stack_reduce%s_kernel<%s>/%s" % ("_bwd" if backward else "", "vector" if vector else "scalar", case.reduction)


def plane_loop(T):
    """(trips of the four-plane loop, planes left to the remainder loop) of stack_reduce_kernel."""
    return T // 4, T % 4


def grid_trips(case):
    """Trips of the grid-stride loop of the kernel a case launches."""
    if case.family == "stack":
        n = numel(case.shape)
        items, cap = (n // 4 if stack_arm(case).find("vector") >= 0 else n), STACK_GRID_CAP
    else:
        B, C, HW = as_bchw(case.shape, case.act, case.dim)
        arm, cap = ensemble_arm(case), ENSEMBLE_GRID_CAP
        if arm.startswith("ensemble_softmax_kernel"):
            items = B * HW // (4 if C <= 8 else 2)
        elif arm.startswith("ensemble_softmax_generic"):
            items = B * HW
        else:
            items = B * C * HW // 4 if arm.startswith("ensemble_kernel") else B * C * HW
    return -(-items // (cap * 256))


# ------------------------------------------------------------------------------------------------- inputs
CLAMP_PROBES = (0.0, 1.0, 1e-9, 0.9999999)          # both clamps of hmean / logodd at the default eps; none negative (gmean, log1p)
EPS_PROBES = (5e-4, 0.9995, 0.01, 0.99)             # clearly on either side of the bounds of eps = 1e-3 and eps = 0.05
SATURATING = (40.0, -60.0)
BOUNDED_LOGIT = 4.0                                 # gmean / logodd of activated logits are compared only for |logit * temperature| <= 4


def bounded(case):
    """gmean and logodd amplify the float32 rounding of a saturated probability (1 - p of p = 0.9999 carries 6e-4; the log of an
    underflowing softmax is unbounded): against the float64 model they get logits with |logit * temperature| <= 4, and the saturating
    rows go to the property checks of the ``props_only`` cases."""
    return case.act is not None and case.reduction in ("gmean", "logodd") and not case.props_only


def inputs(case):
    """The T float32 inputs of a case ([T, *shape] for the stack family), a function of the case only.

    No activation: probabilities in [0.01, 0.99]; CLAMP_PROBES at the first positions of plane 0 and of the last plane, EPS_PROBES behind
    them when the case sets its own eps.  Activations: logits randn * 3 with a run of +40 in plane 0 and a run of -60 in the last plane
    (softmax: in one channel of one pixel each), or bounded logits -- see bounded()."""
    rng = np.random.default_rng(1000 + case.seed)
    n = numel(case.shape)
    if case.act is None:
        x = (rng.random((case.T, n), dtype=np.float32) * np.float32(0.98) + np.float32(0.01)).astype(np.float32)
        probes = CLAMP_PROBES + (EPS_PROBES if case.eps != DEFAULT_EPS else ())
        for t, at in ((0, 0), (case.T - 1, len(probes))):
            k = min(len(probes), max(n - at, 0))
            x[t, at:at + k] = np.asarray(probes[:k], dtype=np.float32)
        x = x.reshape((case.T,) + case.shape)
    else:
        B, C, HW = as_bchw(case.shape, case.act, case.dim)
        x = (rng.standard_normal((case.T, C, B * HW)) * 3).astype(np.float32)       # (channel, pixel) planes: the rows are easy to place
        if bounded(case):
            lim = np.float32(BOUNDED_LOGIT / case.temperature)
            x = np.clip(x, -lim, lim)
        else:
            run = min(4, B * HW)
            x[0, 0, :run] = SATURATING[0]
            x[case.T - 1, C - 1, B * HW - run:] = SATURATING[1]
        if case.act == "softmax":
            d = case.dim % len(case.shape)
            rest = case.shape[:d] + case.shape[d + 1:]
            x = np.moveaxis(x.reshape((case.T, C) + rest), 1, d + 1)
        x = np.ascontiguousarray(x.reshape((case.T,) + case.shape), dtype=np.float32)
    if case.dtype != "float32":
        x = round_to(x, case.dtype)
    return x if case.family == "stack" else [x[t] for t in range(case.T)]


def round_to(x, dtype):
    """float32 values that are exact in the half / bfloat16 source type (what the kernel reads after the widening)."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).to(getattr(torch, dtype)).float().numpy()


def model(case, xs=None):
    """float64 model of a case on its own inputs."""
    xs = inputs(case) if xs is None else xs
    return NO.ensemble64(list(xs), case.reduction, case.act, case.temperature, case.dim, case.eps)


def list_order_sum(xs):
    """float32 sum of the inputs in list order: the bits ``sum`` must give (__fadd_rn in ensemble_kernel, sequential adds over t in
    stack_reduce_kernel)."""
    s = np.asarray(xs[0], dtype=np.float32).copy()
    for x in xs[1:]:
        s = (s + np.asarray(x, dtype=np.float32)).astype(np.float32)
    return s


def reference_chain_f32(case, xs=None):
    """The reference's own float32 evaluation of a case (torch float32 on the CPU, op for op): activation, torch.stack, reduction."""
    import torch

    xs = inputs(case) if xs is None else xs
    acts = [NO.torch_activate(torch.from_numpy(np.ascontiguousarray(x)), case.act, case.temperature, case.dim) for x in xs]
    return NO.torch_chain(torch.stack(acts), case.reduction, case.eps).numpy()


def grad_weights(shape):
    """Upstream gradient of the gradient checks: arange % 5 + 1, fixed and non-constant."""
    return (np.arange(numel(shape), dtype=np.float32).reshape(shape) % 5 + 1).astype(np.float32)


def ratio(got, ref, rtol, atol):
    """Largest |got - ref| / (atol + rtol |ref|) over all elements (NaN where exactly one side is NaN; a NaN on both sides or an equal
    infinity counts as zero error)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref) / (atol + rtol * np.abs(ref))
    same = (np.isnan(got) & np.isnan(ref)) | (got == ref)
    err = np.where(same, 0.0, err)
    return float("nan") if np.isnan(err).any() else float(err.max())


# ------------------------------------------------------------------------------------------------- the tables
# n = 4 * 67: one ragged workgroup of 16-byte lanes; 4 * 300: two workgroups; 4 * 67 + 1: the scalar arm by size; 4 * 67 at an offset of
# one element: the scalar arm by alignment
ONE_GROUP, TWO_GROUPS, ODD = (4, 67), (4, 300), (4 * 67 + 1,)
TEMPERATURES = (1.0, 0.5, 3.0)
ACTS2 = (None, "sigmoid")


def _elementwise():
    cases, k = [], 0

    def add(*a, **kw):
        nonlocal k
        cases.append(make_case("elementwise", *a, seed=k, temperature=TEMPERATURES[k % 3] if kw.get("act") else 1.0, **kw))
        k += 1

    for act in ACTS2:
        for red in REDUCTIONS:                                   # every reduction in the vector and in the scalar arm
            add(ONE_GROUP, 3, red, act=act)
            add(ODD, 3, red, act=act)
        for T in (1, 2, 8, 16):                                  # list lengths, one reduction per OPK, two workgroups
            for red in ("mean", "gmean", "hmean"):
                add(TWO_GROUPS, T, red, act=act)
        for T, red in ((2, "mean"), (16, "logodd"), (1, "sum"), (3, "harmonic1p")):
            add(ONE_GROUP, T, red, act=act, offset=1)            # one input off the 16-byte grid
        for red in ("sum", "gmean", "log1p"):
            add(TWO_GROUPS, 8, red, act=act, scalar=1)           # ptb_set_tunable(1, 1)
    for red in ("gmean", "logodd"):                              # saturating logits: properties only
        add(ONE_GROUP, 3, red, act="sigmoid", props_only=True)
        add(ODD, 3, red, act="sigmoid", props_only=True)
    return cases


def _softmax():
    cases, k = [], 0

    def add(shape, T, red, **kw):
        nonlocal k
        kw.setdefault("temperature", TEMPERATURES[k % 3])
        cases.append(make_case("softmax", shape, T, red, act="softmax", seed=100 + k, **kw))
        k += 1

    Ts = (1, 2, 5, 16)
    for i, C in enumerate((1, 2, 4, 5, 8, 9, 12, 16)):           # both sides of every register bucket (4 / 8 / 16)
        for j, red in enumerate(("mean", "gmean")):
            add((2, C, 6, 6), Ts[(i + j) % 4], red)              # B = 2, HW = 36
            add((3, C, 18, 20), Ts[(i + j + 2) % 4], red)        # B = 3, HW = 360: more than 256 lanes of work
    for C in (3, 7, 13):                                         # every reduction once per bucket
        for red in REDUCTIONS:
            add((3, C, 18, 20), 5, red)
    for red in REDUCTIONS:                                       # the generic kernel: by C ...
        add((2, 17, 6, 6), 3, red)
    for red in ("mean", "gmean", "hmean"):
        add((2, 5, 5, 7), 2, red)                                # ... by HW = 35 ...
        add((2, 5, 6, 6), 5, red, offset=1)                      # ... by alignment ...
        add((2, 9, 6, 6), 2, red, scalar=1)                      # ... and by the tunable
    # softmax over dim 0, 1, 2, -1 of 3-D and 4-D shapes: every bucket through a dim other than 1; dim -1 is HW = 1 (generic)
    for shape, dim in (((3, 10, 8), 0), ((6, 7, 12), 1), ((5, 8, 13), -1), ((7, 2, 4, 6), 0), ((13, 3, 4, 5), 0), ((2, 3, 11, 8), 2),
                       ((2, 3, 4, 12), -1), ((16, 5, 4), 0)):
        for red in ("mean", "gmean"):
            add(shape, 2, red, dim=dim)
    for shape in ((2, 3, 6, 6), (2, 13, 6, 6), (2, 17, 6, 6)):   # saturating logits: properties only
        for red in ("gmean", "logodd"):
            add(shape, 3, red, props_only=True)
    return cases


def _stack():
    cases, k = [], 0

    def add(shape, T, red, **kw):
        nonlocal k
        cases.append(make_case("stack", shape, T, red, seed=200 + k, **kw))
        k += 1

    for T in (2, 3, 4, 5, 8):                                    # short stacks reach this file only with a caller's eps
        for red in ("hmean", "logodd"):
            for eps in (1e-3, 0.05):
                add(ONE_GROUP, T, red, eps=eps)
                add(ODD, T, red, eps=eps)
    for red in ("hmean", "logodd"):
        for eps in (1e-3, 0.05):
            add(TWO_GROUPS, 5, red, eps=eps)
            add(ONE_GROUP, 5, red, eps=eps, offset=1)
            add(ONE_GROUP, 13, red, eps=eps)
    for T in (9, 10, 12, 13, 16, 17):                            # 2, 2, 3, 3, 4, 4 trips of the four-plane loop; remainders 1, 2, 0, 1, 0, 1
        for red in REDUCTIONS:
            add(ONE_GROUP, T, red)
            add(ODD, T, red)
    for red in REDUCTIONS:
        add(TWO_GROUPS, 9, red)
        add(TWO_GROUPS, 17, red)
        add(ONE_GROUP, 10, red, offset=1)
        add(ONE_GROUP, 12, red, scalar=1)
    return cases


ELEMENTWISE, SOFTMAX, STACK = _elementwise(), _softmax(), _stack()

# half / bfloat16 sources through Ensembler: evaluated in float32, rounded once to the source type
LOW_PRECISION = [make_case("elementwise" if act != "softmax" else "softmax", (2, 5, 6, 6), 3, red, act=act, temperature=0.5 if act else 1.0,
                       dtype=dtype, seed=300 + i)
                 for i, (act, red, dtype) in enumerate((a, r, d) for a in (None, "sigmoid", "softmax") for r in ("mean", "gmean")
                                                       for d in ("float16", "bfloat16"))]

ALL = ELEMENTWISE + SOFTMAX + STACK + LOW_PRECISION
ids = lambda c: c.name  # noqa: E731

# one case per capped grid whose grid-stride loop makes a second trip (inputs are drawn on the device; the reference is torch float64 there)
SECOND_TRIP_STACK = make_case("stack", (4 * (STACK_GRID_CAP * 256 + 300),), 2, "hmean", eps=1e-3)
SECOND_TRIP_SOFTMAX = make_case("softmax", (4, 2, ENSEMBLE_GRID_CAP * 256 + 300), 2, "mean", act="softmax", dim=1)    # B * HW = 4 * (cap * 256 + 300)
TAIL = 1200

# every arm the tables must reach (tests/test_ensemble_sweep_cpu.py::test_tables_reach_every_arm)
ARMS = (
    ["ensemble_kernel<OPK=%d,ACT=%d>" % (o, a) for o in (0, 1, 2) for a in (0, 1)]
    + ["ensemble_scalar_kernel<ACT=%d>[%s]" % (a, why) for a in (0, 1) for why in ("size", "alignment", "tunable")]
    + ["ensemble_softmax_kernel<OPK=%d,CREG=%d>" % (o, c) for o in (0, 1, 2) for c in (4, 8, 16)]
    + ["ensemble_softmax_generic_kernel[%s]" % why for why in ("C", "HW", "alignment", "tunable")]
    + ["stack_reduce%s_kernel<%s>/%s" % (b, v, r) for b in ("", "_bwd") for v in ("vector", "scalar") for r in REDUCTIONS]
)
