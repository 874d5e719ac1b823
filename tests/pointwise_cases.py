"""Case tables shared by the sweep of the elementwise and bi-tempered loss kernels (tests/test_pointwise_sweep_cpu.py,
tests/test_pointwise_sweep_gpu.py): csrc/ptb_pointwise.hip behind the autograd Functions of losses/_pointwise.py, called directly so that
flags, parameters and upstream gradients are free -- and through ``_native.launch`` where a Function cannot reach an arm (an output or an
upstream map at an element offset: the Functions allocate those themselves).

A case holds the family (``PointwiseSums`` with its kind 0-5, ``BalancedElementwise``, ``SoftCESums``, ``BiTemperedBinarySums``,
``BiTemperedRows``), the sizes, flags and parameters, the element offset of every tensor inside its allocation, tunables 1 (scalar
kernels) and 4 (the loss grid cap) and a seed; its inputs are a function of the case only.  ``forward_arm`` / ``backward_arm`` restate the
host dispatch (pw_vec, with_pw_kind, launch_sce, the bi-tempered launches) in plain Python and name the kernel instance a case launches,
template arguments spelled as in the .hip file; ``entry_points`` names the C entry points.  The CPU file checks the tables against the
compiler's own list of instances, the GPU file against the kernels the runtime's launch log names.  A handful of ``module`` cases go
through the public classes, so that the scalar algebra around the sums (mean, normalised QFL, class-balance weights, the F1 tail) is
covered too."""
import math
from collections import namedtuple

import numpy as np

from oracle import pointwise_oracle as PO

SOFT_BCE, BALANCED_BCE, QFL, WING, LOGCOSH, SOFT_F1 = range(6)
F_IGNORE, F_SMOOTH = 1, 2
KIND_NAMES = ("soft_bce", "balanced_bce", "qfl", "wing", "logcosh", "soft_f1")
SUM_SLOTS = 64
GRID_CAP = 8192                                 # pw_grid: the default cap of workgroups (tunable 4 replaces it)
ROWS_GRID = 256 * 8                             # ptb_bitempered_rows: workgroups of four rows

TOL = dict(rtol=1e-5, atol=1e-5)                # the north-star bound; sums: atol * max(1, |model|)
GRAD_TOL = dict(rtol=2e-5, atol=1e-5)           # tests/test_losses2_gpu.py test_golden_values_and_gradients
BT_GRAD_TOL = dict(rtol=1e-4, atol=1e-5)        # the golden tests of the bi-tempered kernels
KNIFE = 1e-4                                    # t2 < 1: pixels / rows whose smallest |mass - 1| is below it are left out ...
KNIFE_CAP = 0.01                                # ... and at most this share of a case's pixels / rows may be
EDGE = 1e-3                                     # no element within this of a branch point, unless a case puts it exactly on one

FAMILIES = ("PointwiseSums", "BalancedElementwise", "SoftCESums", "BiTemperedBinarySums", "BiTemperedRows")
DEFAULT_TUN = (0, 0)
TUN_KEYS = (1, 4)

Case = namedtuple("Case", "family name kind B C HW flags p ignore chan elem eps labels t1 t2 smoothing soft off tun seed extreme tag module")

_seed = [0]


def make_case(family, B=1, C=1, HW=1, kind=-1, flags=0, p=(0.0, 0.0, 0.0), ignore=None, chan="", elem=False, eps=0.0, labels="rand", t1=1.0,
              t2=1.0, smoothing=0.0, soft=False, off=(), tun1=0, tun4=0, extreme=False, tag="", module=None):
    """``B, C, HW``: PointwiseSums / BalancedElementwise / BiTemperedBinarySums take n = B * C * HW flat elements (C and HW reach the
    kernel only with per-channel weights, ``chan`` in "w", "pw", "wpw"); SoftCESums [B, C, HW] logits; BiTemperedRows R = B rows of K = C
    classes.  ``ignore``: the ignore value / label handed to the kernel (None: none).  ``labels`` (soft CE): "rand", "absent" (the last
    class never occurs), "some" (some pixels ignored) or "image" (the last image wholly ignored).  ``off``: pairs (tensor, element
    offset)."""
    _seed[0] += 1
    if ignore is not None and family in ("PointwiseSums", "BalancedElementwise"):
        flags |= F_IGNORE
    head = family if kind < 0 else KIND_NAMES[kind]
    if module is not None:
        head = module[0] + "/" + head
    name = "%s-%dx%dx%d" % (head, B, C, HW)
    name += "".join(s for s, on in (("-f%d" % flags, flags), ("-p%g,%g" % (p[0], p[1]), any(p)), ("-ign%g" % (ignore or 0), ignore is not None),
                                    ("-" + chan, chan), ("-elem", elem), ("-eps%g" % eps, eps), ("-" + labels, labels != "rand"),
                                    ("-t%g,%g" % (t1, t2), family.startswith("BiTempered")), ("-s%g" % smoothing, smoothing), ("-soft", soft),
                                    ("-off:" + ",".join("%s%d" % kv for kv in off), off), ("-t1", tun1), ("-t4=%d" % tun4, tun4),
                                    ("-extreme", extreme), ("-" + tag, tag)) if on)
    return Case(family, name, kind, B, C, HW, flags, tuple(float(v) for v in p), ignore, chan, elem, float(eps), labels, float(t1), float(t2),
                float(smoothing), soft, tuple(off), (tun1, tun4), _seed[0], extreme, tag, module)


def numel(case):
    return case.B * case.C * case.HW


def off_of(case, name):
    return dict(case.off).get(name, 0)


def direct(case):
    """The case needs ``_native.launch``: a tensor the Function would allocate itself sits at an element offset."""
    return any(k in ("out", "grad", "grad_elem", "pix_out", "grad_pix") for k, _v in case.off)


def kernel_chw(case):
    """(C, HW) as the host hands them to the point-wise entry points: 1, 1 without per-channel weights."""
    return (case.C, case.HW) if case.chan else (1, 1)


# ------------------------------------------------------------------------------------------------- the host dispatch, restated
def _b(v):
    return "true" if v else "false"


def _bucket(C, *sizes):
    """with_at_most<sizes...>: the first bucket that holds C."""
    for s in sizes:
        if C <= s:
            return s
    raise AssertionError(C)


def _al(case, name, item=4):
    return (off_of(case, name) * item) % 16 == 0


def pw_vec(case, backward):
    """pw_vec(a, extra): the 16-byte arm needs n % 4 == 0, every tensor the launch touches on the 16-byte grid and, with per-channel
    weights, HW % 4 == 0.  Forward: x, t and the optional element-wise output; apply: x, t, the output and the optional upstream map."""
    if case.tun[0] or numel(case) % 4 or not _al(case, "x") or not _al(case, "t"):
        return False
    if case.family == "BalancedElementwise":
        touched = ("grad", "grad_elem") if backward else ("out",)
    elif backward:
        touched = ("grad",) + (("grad_elem",) if case.elem else ())
    else:
        touched = ("out",) if case.elem else ()
    if not all(_al(case, k) for k in touched):
        return False
    return not (case.chan and case.HW % 4)


def sce_vec(case, backward):
    """launch_sce: HW % 4 == 0 and logits, labels (int64), the optional per-pixel output / the gradient and the optional upstream map
    on the 16-byte grid."""
    if case.tun[0] or case.HW % 4 or not _al(case, "x") or not _al(case, "labels", 8):
        return False
    touched = (("grad",) + (("grad_pix",) if case.elem else ())) if backward else (("pix_out",) if case.elem else ())
    return all(_al(case, k) for k in touched)


def _arm(case, backward):
    fam = case.family
    if fam == "PointwiseSums":
        v = _b(pw_vec(case, backward))
        return "pw_apply_kernel<%d,%s,false>" % (case.kind, v) if backward else "pw_fwd_kernel<%d,%s>" % (case.kind, v)
    if fam == "BalancedElementwise":
        arm = "pw_apply_kernel<1,%s,%s>" % (_b(pw_vec(case, backward)), _b(not backward))
        if case.module is not None and not backward:       # balanced_binary_cross_entropy_with_logits(reduction="none"): the counts first
            arm = "pw_fwd_kernel<1,%s>+" % _b(pw_vec(case._replace(family="PointwiseSums", elem=False), False)) + arm
        return arm
    if fam == "SoftCESums":
        mode = 1 if backward else 0
        if case.C > 16:
            return "soft_ce_generic_kernel<%d>" % mode
        return "soft_ce_kernel<%d,%d,%d>" % (4 if sce_vec(case, backward) else 1, _bucket(case.C, 4, 8, 16), mode)
    if fam == "BiTemperedBinarySums":
        return "bitempered_binary_kernel<%s>" % _b(backward)
    assert fam == "BiTemperedRows", fam
    return "bitempered_rows_kernel<%s>" % _b(backward)


def forward_arm(case):
    """The kernel instance(s) the forward of a case launches ("a+b": two launches)."""
    return _arm(case, False)


def backward_arm(case):
    return _arm(case, True)


def entry_points(case):
    """The C entry points a case calls, forward then backward (finalize launches included)."""
    fam = case.family
    fin = [] if direct(case) else ["ptb_sums_finalize"]
    if fam == "PointwiseSums":
        return ["ptb_pointwise_loss_fwd"] + fin + ["ptb_pointwise_loss_apply"]
    if fam == "BalancedElementwise":
        head = ["ptb_pointwise_loss_fwd", "ptb_sums_finalize"] if case.module is not None else []
        return head + ["ptb_pointwise_loss_apply", "ptb_pointwise_loss_apply"]
    if fam == "SoftCESums":
        return ["ptb_soft_ce_fwd"] + fin + ["ptb_soft_ce_bwd"]
    if fam == "BiTemperedBinarySums":
        return ["ptb_bitempered_binary_fwd"] + fin + ["ptb_bitempered_binary_bwd"]
    return ["ptb_bitempered_rows", "ptb_bitempered_rows"]


def launches(case):
    """Counted native calls of forward + backward (``ptb_sums_finalize`` is not counted)."""
    return sum(1 for e in entry_points(case) if e != "ptb_sums_finalize")


def forward_groups(case):
    """(work groups of the forward kernel, elements / pixels per group): a thread takes one group per step of its grid-stride loop."""
    fam = case.family
    if fam in ("PointwiseSums", "BalancedElementwise"):
        pix = 4 if pw_vec(case, False) else 1
        return -(-numel(case) // pix), pix
    if fam == "SoftCESums":
        pix = 4 if (case.C <= 16 and sce_vec(case, False)) else 1
        return case.B * -(-case.HW // pix), pix
    if fam == "BiTemperedBinarySums":
        return numel(case), 1
    return case.B, 1


def forward_grid(case):
    """Workgroups of the forward launch: pw_grid (256 groups a workgroup, capped), four rows a workgroup for the row kernel."""
    groups, _pix = forward_groups(case)
    if case.family == "BiTemperedRows":
        return min(-(-groups // 4), ROWS_GRID)
    return max(1, min(-(-groups // 256), case.tun[1] or GRID_CAP))


def forward_trips(case):
    """(steps of the grid-stride loop the busiest thread makes, groups in the last, partly filled step)."""
    groups, _pix = forward_groups(case)
    per = forward_grid(case) * (4 if case.family == "BiTemperedRows" else 256)
    return -(-groups // per), groups % per


def slot_of(case):
    """The slot (workgroup % SUM_SLOTS) every element / pixel of a case adds into, in the order of the flat inputs (pixels of soft CE:
    [B, HW])."""
    groups, pix = forward_groups(case)
    grid = forward_grid(case)
    if case.family == "SoftCESums":
        gpi = -(-case.HW // pix)
        g = (np.arange(case.B)[:, None] * gpi + np.arange(case.HW)[None, :] // pix).reshape(-1)
    else:
        g = np.arange(numel(case)) // pix
    return ((g % (grid * 256)) // 256) % SUM_SLOTS


def slot_sums(case, parts):
    """[SUM_SLOTS, 4] float64: the workspace a forward must leave, from the per-element contributions ``parts`` [k, n]."""
    out = np.zeros((SUM_SLOTS, 4))
    s = slot_of(case)
    for k, row in enumerate(np.asarray(parts, dtype=np.float64)):
        np.add.at(out[:, k], s, row.reshape(-1))
    return out


# ------------------------------------------------------------------------------------------------- inputs
def wing_constant(case):
    return case.p[0] - case.p[0] * math.log(1 + case.p[0] / case.p[1])


def kernel_params(case):
    """(p0, p1, p2) as the host wrappers hand them over (wing: width, curvature and the constant that joins the branches)."""
    if case.kind == WING:
        return (case.p[0], case.p[1], float(wing_constant(case)))
    return case.p


def _extreme_index(rng, n):
    return rng.choice(n, size=max(n // 16, 1), replace=False) if n >= 4 else np.zeros(0, dtype=np.int64)


def _push_off(v, centre, width=EDGE):
    """Move the elements of ``v`` that lie within ``width`` of ``centre`` to 2 * width from it (same side)."""
    near = np.abs(v - centre) < 2 * width
    return np.where(near, centre + np.where(v >= centre, 4 * width, -4 * width), v).astype(np.float32)


SUPPORT_MARGIN = 0.02                           # t2 < 1: no class has 1 + (1 - t2) (a - norm) within this of 0 (the end of the support)


def support_distance(a, t2):
    """[R, K] float64: 1 + (1 - t2) (a_k - max a - norm) of the float64 model -- 0 is the end of the finite support, where exp_t's
    clamp is a branch point (and for t2 <= t1 the gradient is singular or jumps)."""
    n = np.asarray(a, dtype=np.float64)
    n = n - n.max(axis=1, keepdims=True)
    return 1.0 + (1.0 - t2) * (n - PO.bitempered_rows(a, np.zeros_like(a), 0.5, t2)["norm"])


def _clear_support(a, t2):
    """Rows of float32 activations for t2 < 1 with no class at a branch point: neither on the bound that counts the classes inside the
    support (a - max a == -1 / (1 - t2), ``EDGE``) nor at the end of the support itself (``SUPPORT_MARGIN``); classes that are get moved
    further down (never the row maximum), until none is left."""
    edge = np.float32(-1.0 / (1.0 - t2))
    for _ in range(8):
        top = a.max(axis=1, keepdims=True)
        a = (_push_off(a - top, edge) + top).astype(np.float32)
        near = np.abs(support_distance(a, t2)) < 1.5 * SUPPORT_MARGIN
        if not near.any():
            return a
        a = np.where(near, a - np.float32(4 * SUPPORT_MARGIN / (1.0 - t2)), a).astype(np.float32)
    raise AssertionError("could not clear the support edges")


def _bisection_rows(a, t2):
    """``_clear_support``; a case of fewer than 500 rows could hardly afford a knife edge under ``KNIFE_CAP``, so its rows that come
    near one (smallest |mass - 1| below 4 * KNIFE) are stretched about their maximum until none does."""
    a = _clear_support(a, t2)
    for _ in range(8):
        if a.shape[0] >= 500:
            return a
        near = PO.bitempered_rows(a, np.zeros_like(a), 0.5, t2)["knife"] < 4 * KNIFE
        if not near.any():
            return a
        top = a.max(axis=1, keepdims=True)
        a = _clear_support(np.where(near[:, None], top + (a - top) * np.float32(1.03), a).astype(np.float32), t2)
    raise AssertionError("could not move the rows off the knife edges")


def inputs(case):
    """dict(x, t, labels, chan_w, chan_pw, w): float32 (int64 labels) arrays of a case, a function of the case only.
    Extreme cases: about one element in 16 has |logit| in [20, 80] (point-wise: |x|; wing / log-cosh: |x - t|; soft CE: single logits;
    bi-tempered binary: |x|), the rest is tame."""
    rng = np.random.default_rng(7000 + case.seed)
    fam, n = case.family, numel(case)
    out = dict(x=None, t=None, labels=None, chan_w=None, chan_pw=None, w=None)
    if fam == "SoftCESums":
        B, C, HW = case.B, case.C, case.HW
        x = (rng.standard_normal((B, C, HW)) * 2.5).astype(np.float32)
        if case.extreme:
            idx = _extreme_index(rng, x.size)
            x.reshape(-1)[idx] = (rng.uniform(20, 80, idx.size) * rng.choice([-1.0, 1.0], idx.size)).astype(np.float32)
        lab = rng.integers(0, max(C - 1, 1) if case.labels == "absent" else C, size=(B, HW)).astype(np.int64)
        if case.labels in ("some", "image"):
            lab[rng.random((B, HW)) < 0.3] = case.ignore
            lab[0, 0] = case.ignore
            if case.labels == "image":
                lab[B - 1] = case.ignore
        out.update(x=x, labels=lab)
        return out
    if fam == "BiTemperedRows" and case.tag == "tie":
        # an exact tie of the bisection, placed on purpose: t2 = 0.5, nine classes inside the support give the bracket [0, 4/3]; its second
        # midpoint is 1 (the sum 4/3 + 2/3 rounds to 2), where four classes at the maximum hold 0.5^2 each and five classes one below it
        # hold exactly nothing: mass == 1, and `mass < 1` must send the bisection upwards.  (Exact in float64 and in the row kernel on the
        # MI355X; a float32 bracket one ulp lower gives a mass just above 1 and the same branch -- see the CPU file's check of this case.)
        row = np.array([0, 0, 0, 0, -1, -1, -1, -1, -1], dtype=np.float32) + np.float32(0.5)
        out.update(x=np.ascontiguousarray(np.stack([row, row[::-1], row + np.float32(3.0)])), t=np.eye(9, dtype=np.float32)[[1, 7, 2]])
        return out
    if fam == "BiTemperedRows":
        R, K = case.B, case.C
        x = (rng.standard_normal((R, K)) * 3.0).astype(np.float32)
        if case.soft:
            e = np.exp(rng.standard_normal((R, K)) * 2.0)
            y = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
        else:
            y = np.zeros((R, K), dtype=np.float32)
            y[np.arange(R), rng.integers(0, K, R)] = 1.0
        if case.t2 < 1.0:
            x = _bisection_rows(x, case.t2)
        out.update(x=x, t=y)
        return out
    kind = case.kind
    x = (rng.standard_normal(n) * (3.0 if fam == "BiTemperedBinarySums" or kind in (WING, SOFT_F1) else 2.0)).astype(np.float32)
    ext = _extreme_index(rng, n) if case.extreme else np.zeros(0, dtype=np.int64)
    big = (rng.uniform(20, 80, ext.size) * rng.choice([-1.0, 1.0], ext.size)).astype(np.float32)
    hard = (rng.random(n) < 0.4).astype(np.float32)
    if fam == "BiTemperedBinarySums":
        # (t2 == 1: exp(-2 |x|) must stay a normal float32, or 0 * log(0) turns up where float64 has 0 * log(1e-70))
        x[ext] = big if case.t2 != 1.0 else np.clip(big, -40.0, 40.0)
        if case.t2 < 1.0:                       # rows (-|x|, |x|)
            a = _bisection_rows(np.stack([-np.abs(x), np.abs(x)], axis=1), case.t2)
            x = (np.where(x < 0, -1.0, 1.0) * (a[:, 1] - a[:, 0]) * 0.5).astype(np.float32)
        t = hard
    elif kind in (SOFT_BCE, BALANCED_BCE) or fam == "BalancedElementwise":
        x[ext] = big
        t = rng.random(n).astype(np.float32) if case.soft else hard
    elif kind == QFL:
        x[ext] = big
        beta = case.p[0]
        t = np.where(rng.random(n) < 0.5, 0.0, rng.uniform(0.3, 1.0, n)).astype(np.float32)
        # beta <= 1: the gradient is singular / jumps at sigmoid(x) == t -- tame elements keep a distance, extreme ones a target inside (0, 1)
        p = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
        if beta <= 1.0:
            t[ext] = np.where(rng.random(ext.size) < 0.5, 0.25, 0.75).astype(np.float32)
        near = np.abs(p - t) < (0.05 if beta <= 1.0 else EDGE)
        t = np.where(near, (t + np.float32(0.3)) % np.float32(1.0), t).astype(np.float32)
        if case.tag == "on-target":             # sigmoid(x) == t exactly, in every precision
            k = np.arange(3, n, 11)
            x[k], t[k] = 0.0, 0.5
    elif kind in (WING, LOGCOSH):
        t = (rng.standard_normal(n) * 2.0).astype(np.float32)
        x[ext] = t[ext] + big
        if kind == WING:
            width = np.float32(case.p[0])
            d = np.abs(t.astype(np.float64) - x.astype(np.float64))
            bad = (np.abs(d - float(width)) < 4 * EDGE) | (d < 4 * EDGE)
            x = np.where(bad, t + np.float32(0.5) * width, x).astype(np.float32)
            k = np.arange(2, n, 13)             # exactly on d == width: quarters, so that t - x is exact in float32
            x[k] = np.round(x[k] * 4) / 4
            t[k] = x[k] + width * np.where(k % 2 == 0, 1.0, -1.0).astype(np.float32)
    else:
        assert kind == SOFT_F1, case.name
        if case.flags & F_SMOOTH:               # the probabilities-in form
            x = rng.random(n).astype(np.float32)
        else:
            x[ext] = big
            if case.p[0] > 1e-3:                # the clamp edges sigmoid(x) == eps, 1 - eps
                edge = np.float32(math.log((1 - case.p[0]) / case.p[0]))
                x = np.sign(x).astype(np.float32) * _push_off(np.abs(x), edge)
        t = hard
    if case.ignore is not None:
        t = t.copy()
        t[rng.random(n) < 0.2] = case.ignore
        t[:min(3, n - 1)] = case.ignore
    out.update(x=np.ascontiguousarray(x, dtype=np.float32), t=np.ascontiguousarray(t, dtype=np.float32))
    if "w" in case.chan.replace("pw", ""):
        out["chan_w"] = (0.5 + 0.25 * (np.arange(case.C) % 5)).astype(np.float32)
    if "pw" in case.chan:
        out["chan_pw"] = (2.5 - 0.5 * (np.arange(case.C) % 4)).astype(np.float32)
    if fam == "BalancedElementwise":
        out["w"] = np.array([0.7, 0.4], dtype=np.float32)
        if case.module is not None:             # the class-balance weights of balanced_bce.py:27-34, in float32 like the reference
            n_pos, n_neg = np.float32((t == 1).sum()), np.float32((t == 0).sum())
            gamma = np.float32(case.module[1].get("gamma", 1.0))
            pos = (n_neg / (n_pos + n_neg + np.float32(1e-7))) ** gamma
            out["w"] = np.array([pos ** gamma, (np.float32(1.0) - pos) ** gamma], dtype=np.float32)
    return out


def other(case):
    """The same case with other inputs (for the second call of the GPU file)."""
    return case._replace(seed=case.seed + 100003)


def bad_labels(case, inp):
    """The labels of a soft-CE case with one label outside [0, C) that is not the ignore label, in the middle of image 0."""
    lab = inp["labels"].copy()
    lab[0, case.HW // 2] = case.C if case.ignore != case.C else case.C + 1
    return lab


def upstream(case):
    """Seeded upstream gradients, float32: ``sums`` [4] in [0.5, 1.5) (non-unit scalars for the sums), ``elem`` for the element-wise /
    per-pixel / per-row output, ``loss`` the scalar factor of a module's loss (the number of elements: unit-scale coefficients)."""
    rng = np.random.default_rng(9000 + case.seed)
    shape = (case.B, case.HW) if case.family == "SoftCESums" else ((case.B,) if case.family == "BiTemperedRows" else (numel(case),))
    return dict(sums=(rng.random(4) + 0.5).astype(np.float32), elem=(rng.random(shape) + 0.5).astype(np.float32), loss=np.float32(numel(case)))


# ------------------------------------------------------------------------------------------------- the float64 model
def has_map(case):
    """The case returns an element-wise / per-pixel / per-row output."""
    return case.elem or case.family in ("BalancedElementwise", "BiTemperedRows")


def model(case, inp=None, up=None, labels=None):
    """dict of float64 arrays: "sums" (what the Function returns of the sums), "slots" [SUM_SLOTS, 4] (the workspace of the forward),
    "elem" (the map, where the case has one), "grad" (d sum(upstream * outputs) / dx) and "knife" (t2 < 1: per pixel / row)."""
    inp = inputs(case) if inp is None else inp
    up = upstream(case) if up is None else up
    fam = case.family
    ge = up["elem"] if has_map(case) else None
    g = up["sums"].astype(np.float64)
    if fam == "PointwiseSums":
        C, HW = kernel_chw(case)
        p0, p1, p2 = kernel_params(case)
        r = PO.pointwise(case.kind, inp["x"], inp["t"], case.flags, p0, p1, p2, 0.0 if case.ignore is None else case.ignore, inp["chan_w"], inp["chan_pw"],
                         C, HW, g=(g[0], g[1]), g_elem=ge)
        out = dict(sums=r["sums"], slots=slot_sums(case, r["parts"]), grad=r["grad"])
        if case.elem:
            out["elem"] = r["elem"]
        return out
    if fam == "BalancedElementwise":
        r = PO.balanced_elementwise(inp["x"], inp["t"], inp["w"].astype(np.float64), case.flags, 0.0 if case.ignore is None else case.ignore, ge)
        return dict(elem=r["elem"], grad=r["grad"])
    if fam == "SoftCESums":
        r = PO.soft_ce_pixels(inp["x"], inp["labels"] if labels is None else labels, case.eps, case.ignore is not None, case.ignore or 0, g[0], ge)
        out = dict(sums=np.array([r["total"]]), slots=slot_sums(case, [r["nll"], r["smooth"]]), grad=r["grad"], bad=r["bad"])
        if case.elem:
            out["elem"] = r["pix"]
        return out
    if fam == "BiTemperedBinarySums":
        r = PO.bitempered_binary(inp["x"], inp["t"], case.t1, case.t2, case.smoothing, 5, case.ignore is not None, case.ignore or 0.0, g[0], ge)
        out = dict(sums=np.array([r["sum"]]), slots=slot_sums(case, [r["elem"]]), grad=r["grad"], knife=r["knife"], per=r["elem"])
        if case.elem:
            out["elem"] = r["elem"]
        return out
    assert fam == "BiTemperedRows", fam
    r = PO.bitempered_rows(inp["x"], inp["t"], case.t1, case.t2, case.smoothing, 5, ge)
    return dict(elem=r["loss"], grad=r["grad"], knife=r["knife"])


def kept(case, m):
    """Boolean mask over pixels / rows of what the comparison keeps: everything, except for t2 < 1 the knife edges of the bisection
    (``KNIFE``).  Nothing else in the sweep leaves elements out."""
    if "knife" not in m:
        return None
    return m["knife"] >= KNIFE


def expand_kept(case, keep):
    """``kept`` in the shape of the gradient (rows: every class of a row)."""
    return np.broadcast_to(keep[:, None], (case.B, case.C)) if case.family == "BiTemperedRows" else keep


# ------------------------------------------------------------------------------------------------- the reference's chain in torch
def chain(case, dtype, inp=None, labels=None):
    """(outputs, x): the reference's op chain of a case in torch on the CPU, ``x`` a leaf that requires a gradient -- float64 to check the
    model's analytic gradient, float32 as the reference's own evaluation.  Keys "sums" and "elem" as in ``model``.  (The bi-tempered
    chain is this package's host form of the reference's algebra, pinned against the reference's vectors in tests/test_aux_losses_cpu.py;
    it is not the code under test.)"""
    import torch
    import torch.nn.functional as F

    inp = inputs(case) if inp is None else inp
    fam = case.family
    x = torch.from_numpy(inp["x"]).to(dtype).requires_grad_(True)
    out = {}
    if fam == "SoftCESums":
        lab = torch.from_numpy(inp["labels"] if labels is None else labels)
        ig = (lab == case.ignore) if case.ignore is not None else torch.zeros_like(lab, dtype=torch.bool)
        ig = ig | (lab < 0) | (lab >= case.C)
        lp = F.log_softmax(x, dim=1)
        nll = -lp.gather(1, lab.masked_fill(ig, 0)[:, None])[:, 0].masked_fill(ig, 0.0)
        smooth = -lp.sum(dim=1).masked_fill(ig, 0.0)
        out["sums"] = ((1.0 - case.eps) * nll.sum() + (case.eps / case.C) * smooth.sum()).reshape(1)
        if case.elem:
            out["elem"] = (1.0 - case.eps) * nll + (case.eps / case.C) * smooth
        return out, x
    t = torch.from_numpy(inp["t"]).to(dtype)
    if fam == "BiTemperedRows":
        from pytorch_toolbelt_amd.losses.bitempered_loss import bi_tempered_logistic_loss

        out["elem"] = bi_tempered_logistic_loss(x, t, case.t1, case.t2, label_smoothing=case.smoothing, num_iters=5, reduction="none")
        return out, x
    ig = (t == case.ignore) if case.ignore is not None else torch.zeros_like(t, dtype=torch.bool)
    keep = (~ig).to(dtype)
    if fam == "BiTemperedBinarySums":
        from pytorch_toolbelt_amd.losses.bitempered_loss import bi_tempered_logistic_loss

        tt = t.masked_fill(ig, 0.0)
        per = bi_tempered_logistic_loss(torch.stack([-x, x], dim=1), torch.stack([1 - tt, tt], dim=1), case.t1, case.t2, label_smoothing=case.smoothing,
                                        num_iters=5, reduction="none").masked_fill(ig, 0.0)
        out["sums"] = per.sum().reshape(1)
        out["per"] = per
        if case.elem:
            out["elem"] = per
        return out, x
    if fam == "BalancedElementwise":
        w = torch.from_numpy(inp["w"]).to(dtype)
        out["elem"] = -(w[0] * t * F.logsigmoid(x) + w[1] * (1 - t) * F.logsigmoid(-x)).masked_fill(ig, 0.0)
        return out, x
    kind = case.kind
    zero = torch.zeros((), dtype=dtype)
    elem = None
    if kind == SOFT_BCE:
        C, HW = kernel_chw(case)
        c = torch.from_numpy(PO.channel_of(numel(case), C, HW))
        w = torch.from_numpy(inp["chan_w"]).to(dtype)[c] if inp["chan_w"] is not None else None
        pw = torch.from_numpy(inp["chan_pw"]).to(dtype)[c] if inp["chan_pw"] is not None else None
        st = (1 - t) * case.p[0] + t * (1 - case.p[0]) if case.flags & F_SMOOTH else t
        elem = F.binary_cross_entropy_with_logits(x, st, w, pos_weight=pw, reduction="none") * keep
        sums = [elem.sum(), zero, zero, zero]
    elif kind == BALANCED_BCE:
        sums = [(t * F.logsigmoid(x) * keep).sum(), ((1 - t) * F.logsigmoid(-x) * keep).sum(), (t == 1).to(dtype).sum(), (t == 0).to(dtype).sum()]
    elif kind == QFL:
        bce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
        f = (x.sigmoid() - t).abs().pow(case.p[0])
        elem = f * bce
        sums = [elem.sum(), f.sum(), zero, zero]
    elif kind == WING:
        d = (t - x).abs()
        elem = torch.where(d < case.p[0], case.p[0] * torch.log(1 + d / case.p[1]), d - wing_constant(case))
        sums = [elem.sum(), zero, zero, zero]
    elif kind == LOGCOSH:
        z = x - t
        elem = z + F.softplus(-2.0 * z) - math.log(2.0)
        sums = [elem.sum(), zero, zero, zero]
    else:
        p = x if case.flags & F_SMOOTH else x.sigmoid().clamp(case.p[0], 1 - case.p[0])
        p, tt = p * keep, t.masked_fill(ig, 0.0)
        sums = [(p * tt).sum(), p.sum(), tt.sum(), keep.sum()]
    out["sums"] = torch.stack([s.to(dtype) for s in sums])
    if case.elem:
        out["elem"] = elem if elem is not None else torch.zeros_like(x)
    return out, x


def chain_gradient(case, dtype, inp=None, up=None):
    """(outputs as numpy, d sum(upstream * outputs) / dx) of ``chain``."""
    import torch

    up = upstream(case) if up is None else up
    out, x = chain(case, dtype, inp)
    total = 0.0
    for k, v in out.items():
        if k == "per":
            continue
        g = torch.from_numpy(up[k][:v.numel()] if k == "sums" else up[k]).to(dtype)
        total = total + (v * g).sum()
    total.backward()
    return {k: v.detach().numpy() for k, v in out.items()}, x.grad.numpy()


def ratio(got, ref, rtol, atol, scale_atol=False, keep=None):
    """Largest |got - ref| / (atol' + rtol |ref|) over the elements ``keep`` selects (all without it); atol' = atol * max(1, |ref|) for
    sums.  Elements where the model is not finite must agree in position and kind (NaN with NaN, an infinity with the same infinity):
    inf when they do not; NaN when ``got`` is not finite where the model is."""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if keep is not None:
        keep = np.asarray(keep).reshape(-1)
        got, ref = got[keep], ref[keep]
    odd = ~np.isfinite(ref)
    if odd.any():
        same = np.where(np.isnan(ref[odd]), np.isnan(got[odd]), got[odd] == ref[odd])
        if not same.all():
            return float("inf")
        got, ref = got[~odd], ref[~odd]
    if got.size == 0:
        return 0.0
    a = atol * np.maximum(1.0, np.abs(ref)) if scale_atol else atol
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref) / (a + rtol * np.abs(ref))
    return float("nan") if not np.isfinite(err).all() else float(err.max())


def grad_tol(case):
    return BT_GRAD_TOL if case.family.startswith("BiTempered") else GRAD_TOL


def value_ratios(case, got, want, keep=None):
    """{key: worst error / tolerance} of the values of a case.  The counts of balanced BCE and of soft F1 (hard targets) are exact.
    With knife edges left out (``keep``), the sums are compared through the per-element values only (the map, or "per")."""
    r = {}
    some_out = keep is not None and not keep.all()
    for k in ("sums", "slots", "elem", "per"):
        if k not in want or k not in got:
            continue
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        if k in ("sums", "slots"):
            if some_out:
                continue
            r[k] = ratio(g, w[..., :g.shape[-1]] if k == "sums" else w, scale_atol=True, **TOL)
        else:
            r[k] = ratio(g, w, keep=keep, **TOL)
    return r


# ------------------------------------------------------------------------------------------------- the module cases
def module_tail(case, out, n, torch):
    """The scalar algebra of a public class around the sums of its Function, in torch (``out`` as ``chain`` returns it)."""
    cls, kw = case.module
    s = out.get("sums")
    red = kw.get("reduction", "mean")
    if cls == "QualityFocalLoss" and red == "normalized":
        return s[0] / s[1]
    if cls == "BinarySoftF1Loss":
        loss = 1 - 2 * s[0] / (s[1] + s[2] + 1e-6)
        return torch.where(s[3] > 0, loss, torch.zeros_like(loss))
    if cls == "balanced_bce" and red == "mean":
        gamma = kw.get("gamma", 1.0)
        pos = torch.pow((s[3] / (s[2] + s[3] + 1e-7)).detach().float(), gamma)
        return -(pos.pow(gamma).to(s.dtype) * s[0] + (1.0 - pos).pow(gamma).to(s.dtype) * s[1]) / n
    if red == "none":
        return out["elem"]
    if cls == "BiTemperedLogisticLoss":
        return out["elem"].mean()
    if cls == "SoftCrossEntropyLoss":
        return s[0] / (case.B * case.HW)
    return s[0] / n if red == "mean" else s[0]


def module_model(case, inp):
    """The loss of a module case from the reduced float64 functions of oracle/pointwise_oracle.py (not from the per-element model)."""
    cls, kw = case.module
    x, t = inp["x"], inp["t"]
    if cls == "SoftBCEWithLogitsLoss":
        shape = (case.B, case.C, case.HW)
        w = inp["chan_w"].reshape(1, -1, 1) if inp["chan_w"] is not None else None
        pw = inp["chan_pw"].reshape(1, -1, 1) if inp["chan_pw"] is not None else None
        return PO.soft_bce(x.reshape(shape), t.reshape(shape), w, pw, kw.get("ignore_index", -100), kw.get("reduction", "mean"), kw.get("smooth_factor")).reshape(-1)
    if cls == "balanced_bce":
        return np.asarray(PO.balanced_bce(x, t, kw.get("gamma", 1.0), kw.get("ignore_index"), kw.get("reduction", "mean"))).reshape(-1)
    if cls == "QualityFocalLoss":
        return np.asarray(PO.quality_focal(x, t, kw.get("beta", 2.0), kw.get("reduction", "mean"))).reshape(-1)
    if cls == "wing_loss":
        return np.asarray(PO.wing(x, t, kw.get("width", 5), kw.get("curvature", 0.5))).reshape(-1)
    if cls == "log_cosh_loss":
        return np.asarray(PO.log_cosh(x, t)).reshape(-1)
    if cls == "SoftCrossEntropyLoss":
        return np.asarray(PO.soft_ce(x, inp["labels"], kw.get("smooth_factor", 0.0), kw.get("ignore_index", -100), "mean")).reshape(-1)
    if cls == "BinarySoftF1Loss":
        keep = t != kw["ignore_index"] if kw.get("ignore_index") is not None else np.ones(t.shape, dtype=bool)
        eps = kw.get("eps", 1e-6)
        p = np.clip(1.0 / (1.0 + np.exp(-x[keep].astype(np.float64))), eps, 1 - eps)
        tt = t[keep].astype(np.float64)
        tp, fp, fn = (p * tt).sum(), (p * (1 - tt)).sum(), ((1 - p) * tt).sum()
        return np.array([1 - 2 * tp / (2 * tp + fn + fp + 1e-6)])
    if cls == "BinaryBiTemperedLogisticLoss":
        return np.array([PO.bitempered_binary(x, t, kw["t1"], kw["t2"], kw.get("smoothing", 0.0))["sum"] / x.size])
    assert cls == "BiTemperedLogisticLoss", cls
    return np.array([PO.bitempered_rows(x, t, kw["t1"], kw["t2"], kw.get("smoothing", 0.0))["loss"].mean()])


def module_chain_gradient(case, dtype, inp, up):
    """(loss as numpy, d (upstream * loss) / dx) of a module case: ``chain`` of its Function and ``module_tail``."""
    import torch

    out, x = chain(case, dtype, inp)
    loss = module_tail(case, out, numel(case), torch)
    g = torch.from_numpy(up["elem"]).to(dtype) if loss.dim() else float(up["loss"])
    (loss * g).sum().backward()
    return loss.detach().numpy().reshape(-1), x.grad.numpy()


# ------------------------------------------------------------------------------------------------- the tables
TRIP_GROUPS = (1, 255, 256, 257, 512, 513, 769)         # with tunable 4 at 1 the stride is 256 groups
CHAN_SHAPES = ((2, 3, 4), (2, 3, 5), (1, 1, 8), (3, 2, 12), (2, 5, 7))
WING_PARAMS = ((5.0, 0.5), (2.0, 1.0), (3.0, 0.5))
QFL_BETAS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0)
BT_TEMPS = ((0.8, 1.2), (0.7, 0.6), (1.0, 1.0), (1.0, 1.4), (0.5, 1.0), (0.9, 0.9), (1.0, 0.7))


def _kind_kw(kind, i=0):
    """A representative parameter set of each kind (``i`` varies it)."""
    if kind == SOFT_BCE:
        return (dict(), dict(flags=F_SMOOTH, p=(0.1, 0, 0)), dict(ignore=-100.0), dict(flags=F_SMOOTH, p=(0.2, 0, 0), ignore=-100.0, soft=True))[i % 4]
    if kind == BALANCED_BCE:
        return (dict(), dict(ignore=-100.0))[i % 2]
    if kind == QFL:
        return dict(p=(QFL_BETAS[(i + 4) % 6], 0, 0))
    if kind == WING:
        return dict(p=WING_PARAMS[i % 3] + (0.0,))
    if kind == LOGCOSH:
        return dict()
    return (dict(p=(1e-6, 0, 0)), dict(p=(0.05, 0, 0), ignore=255.0), dict(flags=F_SMOOTH), dict(p=(0.05, 0, 0)), dict(flags=F_SMOOTH, ignore=255.0),
            dict(p=(1e-6, 0, 0), ignore=255.0))[i % 6]


def _has_elem(kind):
    return kind in (SOFT_BCE, QFL, WING, LOGCOSH)


def _pointwise():
    cases, add = [], lambda n, **kw: cases.append(make_case("PointwiseSums", 1, 1, n, **kw))
    for kind in range(6):
        # grid-stride tails: one workgroup, 256 groups a step (the vector forward takes two groups a step)
        for i, groups in enumerate(TRIP_GROUPS):
            add(groups * 4, kind=kind, tun4=1, elem=_has_elem(kind) and i % 2 == 0, **_kind_kw(kind, i))
            if groups in (257, 513):
                add(groups, kind=kind, tun4=1, tun1=1, **_kind_kw(kind, i))                 # the scalar kernels, one group an element
        # the slots: 65 and 129 workgroups of the scalar arm, 65 of the vector arm
        add(65 * 256, kind=kind, tun1=1, **_kind_kw(kind, 1))
        add(128 * 256 + 3, kind=kind, **_kind_kw(kind, 2))
        add(65 * 1024, kind=kind, elem=_has_elem(kind), **_kind_kw(kind, 3))
        # vector and scalar arms: n % 4, tunable 1, every tensor at an offset of 1 (scalar) and of 4 elements (vector)
        for i, n in enumerate((1028, 1029, 1031, 3)):
            add(n, kind=kind, elem=_has_elem(kind) and i % 2 == 1, **_kind_kw(kind, i))
        add(1028, kind=kind, tun1=1, elem=_has_elem(kind), **_kind_kw(kind, 0))
        tensors = ("x", "t", "grad") + (("out", "grad_elem") if _has_elem(kind) else ())
        for i, name in enumerate(tensors):
            for o in (1, 4):
                add(1032, kind=kind, elem=_has_elem(kind), off=((name, o),), **_kind_kw(kind, i))
        # values: every parameter set tame and extreme
        for i in range({SOFT_BCE: 4, BALANCED_BCE: 2, QFL: 6, WING: 3, LOGCOSH: 1, SOFT_F1: 6}[kind]):
            for extreme in (False, True):
                if extreme and _kind_kw(kind, i).get("flags", 0) & F_SMOOTH and kind == SOFT_F1:
                    continue                            # probabilities in: there are no logits to be extreme
                add(2052, kind=kind, elem=_has_elem(kind), extreme=extreme, tag="values", **_kind_kw(kind, i))
    for beta in (0.5, 1.0, 0.0, 2.0):               # sigmoid(x) == t exactly: NaN gradients at beta < 1, as in torch
        add(1028, kind=QFL, p=(beta, 0, 0), elem=True, tag="on-target")
        add(1027, kind=QFL, p=(beta, 0, 0), tag="on-target")
    # per-channel weights
    k = 0
    for B, C, HW in CHAN_SHAPES:
        for chan in ("w", "pw", "wpw"):
            for plain in (True, False):
                kw = dict() if plain else dict(flags=F_SMOOTH, p=(0.1, 0, 0), ignore=-100.0)
                cases.append(make_case("PointwiseSums", B, C, HW, kind=SOFT_BCE, chan=chan, elem=k % 2 == 0, **kw))
                k += 1
    cases.append(make_case("PointwiseSums", 2, 3, 4, kind=SOFT_BCE, chan="wpw", tun1=1))
    cases.append(make_case("PointwiseSums", 3, 5, 260, kind=SOFT_BCE, chan="wpw", elem=True, flags=F_SMOOTH, p=(0.1, 0, 0), ignore=-100.0, extreme=True))
    cases.append(make_case("PointwiseSums", 3, 5, 1028, kind=SOFT_BCE, chan="wpw", tun4=1))                  # several steps with weights
    return cases


def _balanced():
    cases, add = [], lambda n, **kw: cases.append(make_case("BalancedElementwise", 1, 1, n, **kw))
    for i, groups in enumerate(TRIP_GROUPS):
        add(groups * 4, tun4=1, ignore=(None, -100.0)[i % 2])
    add(513, tun4=1, tun1=1)
    for i, n in enumerate((1028, 1029, 1031)):
        add(n, ignore=(None, -100.0)[i % 2], extreme=i == 0)
    add(1028, tun1=1)
    for name in ("x", "t", "out", "grad", "grad_elem"):
        for o in (1, 4):
            add(1032, off=((name, o),), ignore=-100.0)
    add(2052, extreme=True, ignore=-100.0)
    return cases


def _soft_ce():
    cases = []

    def add(B, C, HW, **kw):
        if kw.get("labels") in ("some", "image") and kw.get("ignore") is None:
            kw["ignore"] = -100
        cases.append(make_case("SoftCESums", B, C, HW, **kw))

    k = 0
    for C in (1, 2, 4, 5, 8, 9, 16, 17, 33):
        for HW in (1, 3, 4, 8, 260):
            labels = ("rand", "some", "image", "absent")[k % 4]
            if labels == "absent" and C == 1:
                labels = "some"
            add(2, C, HW, eps=(0.0, 0.1, 1.0)[k % 3], labels=labels, elem=k % 2 == 0, extreme=HW == 260 and C in (4, 9, 17), ignore=-100 if k % 5 == 0 else None)
            k += 1
    for C in (4, 5, 8, 9, 16, 17):
        add(2, C, 260, eps=0.1, tun1=1, elem=C % 2 == 0, labels="some")
    # grid-stride tails of the pixel groups (B = 2: two images' groups in one launch)
    for i, groups in enumerate(TRIP_GROUPS):
        half = max(groups // 2, 1)
        B = 2 if groups % 2 == 0 else 1
        add(B, (3, 5, 9)[i % 3], (half if B == 2 else groups) * 4, eps=0.1, tun4=1, elem=i % 2 == 0, labels=("rand", "some")[i % 2])
    add(1, 5, 513, eps=0.1, tun4=1, labels="some")
    add(1, 17, 513, eps=0.1, tun4=1, elem=True)
    add(1, 3, 65 * 256, eps=0.1, tun1=1)             # 65 workgroups: the slots wrap
    # the alignment arms of launch_sce
    for i, name in enumerate(("x", "labels", "pix_out", "grad", "grad_pix")):
        for o in (1, 4):
            add(2, (3, 7, 12)[i % 3], 64, eps=0.1, elem=True, off=((name, o),), labels=("rand", "some")[i % 2])
    add(2, 12, 64, eps=0.1, off=(("x", 1),))
    return cases


def _bt_binary():
    cases, add = [], lambda n, **kw: cases.append(make_case("BiTemperedBinarySums", 1, 1, n, **kw))
    k = 0
    for t1, t2 in BT_TEMPS:
        for smoothing in (0.0, 0.1):
            for ignore in (None, 255.0):
                # (t2 < 1: with knife edges left out the sum is compared through the per-element map, so these cases ask for it)
                add(2052 if k % 2 else 1027, t1=t1, t2=t2, smoothing=smoothing, ignore=ignore, elem=k % 2 == 0 or t2 < 1.0, extreme=k % 4 == 1)
                k += 1
    for i, groups in enumerate(TRIP_GROUPS):
        t1, t2 = BT_TEMPS[i % len(BT_TEMPS)]
        add(groups, t1=t1, t2=t2, tun4=1, elem=i % 2 == 0 or (t2 < 1.0 and groups >= 500), smoothing=(0.0, 0.1)[i % 2])
    add(65 * 256, t1=0.8, t2=1.2)
    add(128 * 256 + 3, t1=0.7, t2=0.6, ignore=255.0, elem=True)
    return cases


def _bt_rows():
    cases, add = [], lambda R, K, **kw: cases.append(make_case("BiTemperedRows", R, K, 1, **kw))
    k = 0
    for K in (1, 2, 63, 64, 65, 129, 257):
        for t1, t2 in BT_TEMPS:
            R = (1, 3, 4, 5)[k % 4]
            if K == 1:
                add(R, K, t1=t1, t2=t2, soft=False)
            else:
                add(R if K > 2 else R * 50, K, t1=t1, t2=t2, smoothing=(0.0, 0.1)[k % 2], soft=bool((k // 2) % 2))
            k += 1
    for i, (t1, t2) in enumerate(BT_TEMPS):
        add(400, (3, 5, 65)[i % 3], t1=t1, t2=t2, smoothing=(0.1, 0.0)[i % 2], soft=i % 2 == 0)       # enough rows for the 1 % cap to mean something
    add(3, 9, t1=0.8, t2=0.5, tag="tie")
    add(8197, 3, t1=0.8, t2=1.2, smoothing=0.1)     # more rows than 4 * ROWS_GRID: the grid-stride loop
    add(8197, 3, t1=0.7, t2=0.6, soft=True)
    return cases


def _modules():
    cases = []

    def add(cls, kw, family, B, C, HW, **ckw):
        cases.append(make_case(family, B, C, HW, module=(cls, kw), **ckw))

    add("SoftBCEWithLogitsLoss", dict(smooth_factor=0.1), "PointwiseSums", 2, 3, 12, kind=SOFT_BCE, chan="wpw", flags=F_SMOOTH, p=(0.1, 0, 0), ignore=-100.0)
    add("SoftBCEWithLogitsLoss", dict(reduction="none", ignore_index=None), "PointwiseSums", 2, 3, 5, kind=SOFT_BCE, chan="w", elem=True)
    add("QualityFocalLoss", dict(reduction="normalized"), "PointwiseSums", 2, 3, 12, kind=QFL, p=(2.0, 0, 0))
    add("QualityFocalLoss", dict(beta=1.5), "PointwiseSums", 2, 3, 11, kind=QFL, p=(1.5, 0, 0))
    add("balanced_bce", dict(gamma=1.5), "PointwiseSums", 2, 3, 12, kind=BALANCED_BCE)
    add("balanced_bce", dict(gamma=0.5, ignore_index=-100, reduction="none"), "BalancedElementwise", 2, 3, 12, ignore=-100.0)
    add("BinarySoftF1Loss", dict(ignore_index=255, eps=0.05), "PointwiseSums", 2, 1, 66, kind=SOFT_F1, p=(0.05, 0, 0), ignore=255.0)
    add("wing_loss", dict(width=2.0, curvature=1.0), "PointwiseSums", 2, 3, 12, kind=WING, p=(2.0, 1.0, 0.0))
    add("log_cosh_loss", dict(), "PointwiseSums", 2, 3, 11, kind=LOGCOSH)
    add("SoftCrossEntropyLoss", dict(smooth_factor=0.1), "SoftCESums", 2, 5, 12, eps=0.1, labels="some", ignore=-100)
    add("BinaryBiTemperedLogisticLoss", dict(t1=0.8, t2=1.2, smoothing=0.1), "BiTemperedBinarySums", 2, 1, 66, t1=0.8, t2=1.2, smoothing=0.1)
    add("BiTemperedLogisticLoss", dict(t1=0.5, t2=1.0, smoothing=0.1), "BiTemperedRows", 12, 6, 1, t1=0.5, t2=1.0, smoothing=0.1)
    return cases


POINTWISE, BALANCED, SOFT_CE, BT_BINARY, BT_ROWS, MODULES = _pointwise(), _balanced(), _soft_ce(), _bt_binary(), _bt_rows(), _modules()
FUNCTIONS = POINTWISE + BALANCED + SOFT_CE + BT_BINARY + BT_ROWS
ALL = FUNCTIONS + MODULES
ids = lambda c: c.name  # noqa: E731


def family_of(case):
    """The row of the worst-ratio tables a case is noted in."""
    if case.module is not None:
        return "module"
    return KIND_NAMES[case.kind] if case.family == "PointwiseSums" else case.family


GROUPS = {}                                     # {row of the worst-ratio tables: its Function cases}: the tests run one group at a time
for _c in FUNCTIONS:
    GROUPS.setdefault(family_of(_c), []).append(_c)


def each(cases, check):
    """Run ``check(case)`` on every case and fail once, naming every case that failed with the first line of its assertion: the suites
    count one test per group of cases, not one per case."""
    failed = []
    for case in cases:
        try:
            check(case)
        except AssertionError as e:
            failed.append("%s: %s" % (case.name, (str(e).strip().splitlines() or ["assertion failed"])[0][:300]))
    assert not failed, "%d of %d cases failed:\n%s" % (len(failed), len(cases), "\n".join(failed[:25]))


def bad_label_cases():
    """One soft-CE case per forward arm (the first of the table that reaches it, through the Function)."""
    seen, out = set(), []
    for case in SOFT_CE:
        arm = forward_arm(case)
        if arm not in seen and not direct(case) and case.HW >= 3:
            seen.add(arm)
            out.append(case)
    return out


# Kernel instances of ptb_pointwise.hip that no case reaches, each with its reason (tests/test_pointwise_sweep_cpu.py fails on an
# instance that is neither reached nor listed here, and on an entry that a case does reach).
UNREACHED = {}
