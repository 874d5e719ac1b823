"""Case tables shared by the sweep of the segmentation-loss kernels (tests/test_seg_loss_sweep_cpu.py, tests/test_seg_loss_sweep_gpu.py):
csrc/ptb_losses.hip behind the autograd Functions of losses/_kernels.py, called directly so that flags and coefficients are free.

A case holds the family (the Function), B, C, HW, the target kind, the activation of the statistics, the focal options, the epilogue
options, the element offset of logits / labels / dense target inside their allocations, tunables 1, 4, 7, 16 and 20 and a seed; its
inputs are a function of the case only.  ``forward_arm`` / ``backward_arm`` restate the host dispatch (seg_loss_fwd_launch, focal_only_pk,
ptb_focal_bwd, ptb_seg_stats_bwd, launch_smf<0 / 1>, ptb_seg_fused_bwd, ptb_region_loss_fwd vs ptb_region_epilogue) in plain Python and
name the kernel instance a case launches, template arguments spelled as in the .hip file -- so that the CPU file can check the tables
against the compiler's own list of instances, and the GPU file can compare them with the kernels the runtime's launch log names (and
``entry_points`` with the C entry points that were called): a move of the real dispatch, or a wrong restatement, fails there."""
from collections import namedtuple

import numpy as np

from oracle import seg_loss_oracle as SO

PROB_SOFTMAX, PROB_SIGMOID, PROB_IDENTITY = SO.PROB_SOFTMAX, SO.PROB_SIGMOID, SO.PROB_IDENTITY
SEG_FOCAL, SEG_STATS, SEG_HAS_IGNORE, SEG_HAS_ALPHA, SEG_REDUCED, SEG_MASK_FOCAL_TERM, SEG_ELEMWISE, SEG_NO_TERM = 1, 2, 4, 8, 16, 32, 64, 128
SUM_SLOTS = 64
GRID_STREAM, GRID_STATS, GRID_FOCAL_PK = 256 * 32, 256 * 8, 512        # kGridStream, kGridStats, kGridFocalPk (workgroups of 4 waves)

TOL = dict(rtol=1e-5, atol=1e-5)                # the north-star bound (tests/test_losses_gpu.py TOL); sums: atol * max(1, |model|)
GRAD_TOL = dict(rtol=2e-4, atol=2e-6)           # gradients on tame pixels  } test_softmax_focal_fast_and_exact_paths_agree_with_fp64
GRAD_TOL_EXTREME = dict(rtol=2e-4, atol=1e-4)   # gradients on extreme pixels }
EXTREME_LOGIT = 60.0                            # a pixel is extreme when max_c |logit| exceeds it (decided from the inputs)

DEFAULT_TUN = (0, 0, 4, 1, 1)                   # tunables 1, 4, 7, 16, 20 as the library starts
TUN_KEYS = (1, 4, 7, 16, 20)

FAMILIES = ("SigmoidFocalSums", "FocalScalar", "RegionStats", "SoftmaxFocalSums", "FusedSegSums", "RegionLoss", "module")

# the scalar tail: focal on / off, the region weights, smooth, eps, log_loss, the selected classes (None = all)
Epi = namedtuple("Epi", "with_focal dice_weight jaccard_weight smooth eps log_loss classes")
Case = namedtuple("Case", "family name B C HW target prob gamma alpha threshold cw ignore ignored elem no_term mask_term epi one_launch "
                          "dtype off tun seed extreme labels module")

_seed = [0]


def make_case(family, B, C, HW, target="labels", prob=PROB_SOFTMAX, gamma=2.0, alpha=None, threshold=None, cw=False, ignore=None,
              ignored=None, elem=False, no_term=False, mask_term=False, epi=None, one_launch=True, off=(0, 0, 0), t1=0, t4=0, t7=4, t16=1,
              t20=1, extreme=False, labels="rand", module=None, tag=""):
    """``target``: "labels" (int64 [B, HW]), "dense" (0 / 1 float32 [B, C, HW]) or "soft" (dense targets in [0, 1]).  ``ignore``: the
    ignore label / value handed to the kernel (None: no ignore flag); ``ignored``: whether the data holds ignored elements (default:
    whenever ``ignore`` is given).  ``off``: element offsets of (logits, labels, dense target).  ``labels``: "rand", "absent" (the last
    class never occurs) or "one" (every pixel in one class)."""
    _seed[0] += 1
    ignored = (ignore is not None) if ignored is None else ignored
    name = "%s-%dx%dx%d-%s-p%d" % (family if module is None else module[0], B, C, HW, target, prob)
    name += "".join(s for s, on in (("-g%g" % gamma, gamma != 2.0), ("-a%g" % (alpha or 0), alpha is not None),
                                    ("-thr%g" % (threshold or 0), threshold is not None), ("-cw", cw), ("-ign%g" % (ignore or 0), ignore is not None),
                                    ("-noign", ignore is not None and not ignored), ("-elem", elem), ("-noterm", no_term), ("-mask", mask_term),
                                    ("-epilogue", not one_launch), ("-off%d%d%d" % tuple(off), any(off)), ("-t1", t1), ("-t4=%d" % t4, t4),
                                    ("-t7=%d" % t7, t7 != 4), ("-t16=0", not t16), ("-t20=0", not t20), ("-extreme", extreme),
                                    ("-" + labels, labels != "rand"), ("-" + tag, tag)) if on)
    if epi is not None:
        name += "-f%d-d%g-j%g-s%g%s%s" % (epi.with_focal, epi.dice_weight, epi.jaccard_weight, epi.smooth, "-log" if epi.log_loss else "",
                                         "-classes" if epi.classes is not None else "")
    return Case(family, name, B, C, HW, target, prob, float(gamma), alpha, threshold, cw, ignore, ignored, elem, no_term, mask_term, epi,
                one_launch, "float32", tuple(off), (t1, t4, t7, t16, t20), _seed[0], extreme, labels, module)


def flags_of(case):
    """The option bits a case hands to its Function (the Function adds SEG_FOCAL / SEG_STATS itself)."""
    return ((SEG_HAS_IGNORE if case.ignore is not None else 0) | (SEG_HAS_ALPHA if case.alpha is not None else 0)
            | (SEG_REDUCED if case.threshold is not None else 0) | (SEG_MASK_FOCAL_TERM if case.mask_term else 0)
            | (SEG_ELEMWISE if case.elem else 0) | (SEG_NO_TERM if case.no_term else 0))


def what_of(case):
    """SEG_FOCAL | SEG_STATS of the forward launch."""
    if case.family in ("SigmoidFocalSums", "FocalScalar"):
        return SEG_FOCAL
    if case.family == "RegionStats":
        return SEG_STATS
    if case.family == "FusedSegSums":
        return SEG_FOCAL | SEG_STATS
    assert case.family == "RegionLoss", case.family
    return SEG_STATS | (SEG_FOCAL if case.epi.with_focal else 0)


# ------------------------------------------------------------------------------------------------- the host dispatch, restated
def _b(v):
    return "true" if v else "false"


def _bucket(C, *sizes):
    """with_at_most<sizes...>: the first bucket that holds C; the last value is the fallback."""
    for s in sizes[:-1]:
        if C <= s:
            return s
    return sizes[-1]


def _aligned(case, *which):
    """16-byte alignment of the tensors a launch reads: every allocation starts on the grid (the GPU file asserts it), so only the
    case's own element offsets count -- float32 logits / dense targets 4 bytes an element, int64 labels 8."""
    ox, ol, od = case.off
    ok = True
    if "logits" in which:
        ok = ok and (ox * 4) % 16 == 0
    if "labels" in which and case.target == "labels":
        ok = ok and (ol * 8) % 16 == 0
    if "dense" in which and case.target != "labels":
        ok = ok and (od * 4) % 16 == 0
    return ok


def vec_ok(case):
    """vec_ok(HW, {logits, dense, labels, <fresh outputs>}) of ptb_loss_device.h."""
    return case.HW % 4 == 0 and not case.tun[0] and _aligned(case, "logits", "labels", "dense")


def _pk(case, term, focal, stats):
    cr = _bucket(case.C, 4, 8, 16)
    full = case.C == cr and not (term and focal and stats)
    return "seg_focal_pk_kernel<%d,%s,%s,%s,%s>" % (cr, _b(term), _b(full), _b(focal), _b(stats))


def _focal_only_pk(case, what):
    f = flags_of(case)
    return (what == SEG_FOCAL and not case.tun[0] and case.tun[4] and case.target == "labels" and case.HW % 128 == 0 and case.C <= 16
            and case.gamma == 2.0 and not case.cw and not (f & (SEG_HAS_ALPHA | SEG_REDUCED | SEG_ELEMWISE | SEG_HAS_IGNORE)) and vec_ok(case))


def _seg_forward(case):
    """seg_loss_fwd_launch."""
    what, f = what_of(case), flags_of(case)
    C, HW, prob = case.C, case.HW, case.prob
    if what == SEG_FOCAL:
        prob = PROB_SIGMOID
    labels, dense = case.target == "labels", case.target != "labels"
    cw = case.cw and bool(what & SEG_FOCAL)                 # RegionStats hands no class weights in
    g2 = case.gamma == 2.0
    scalar, vec = bool(case.tun[0]), vec_ok(case)
    ign = bool(f & SEG_HAS_IGNORE)
    if not scalar and dense and what == 3 and vec and HW % 1024 == 0 and prob == PROB_SIGMOID and g2 and not cw and not (f & (SEG_HAS_ALPHA | SEG_REDUCED | SEG_ELEMWISE)):
        return "seg_stats_dense_lean_kernel<1,%s,true>" % _b(ign)
    if not scalar and dense and what == SEG_STATS and vec and HW % 1024 == 0 and prob in (PROB_SIGMOID, PROB_IDENTITY):
        return "seg_stats_dense_lean_kernel<%d,%s,false>" % (prob, _b(ign))
    if not scalar and labels and vec and HW % 256 == 0 and C <= 16 and (what & SEG_STATS) and not (f & SEG_ELEMWISE) and prob in (PROB_SOFTMAX, PROB_IDENTITY):
        plain_focal = what == 3 and prob == PROB_SOFTMAX and g2 and not cw and not (f & (SEG_HAS_IGNORE | SEG_HAS_ALPHA | SEG_REDUCED))
        stats_pk = prob == PROB_SOFTMAX and not ign and case.tun[4] and HW % 128 == 0
        if what == SEG_STATS or plain_focal:
            if plain_focal:
                return _pk(case, not (f & SEG_NO_TERM), True, True)
            if stats_pk:
                return _pk(case, False, False, True)
            return "seg_fwd_lean_kernel<%d,%d,%s>" % (_bucket(C, 4, 8, 16), prob, _b(ign))
    if _focal_only_pk(case, what):
        return _pk(case, not (f & SEG_NO_TERM), True, False)
    if what == SEG_FOCAL and not scalar and labels and vec and HW % 256 == 0 and g2 and not cw and not (f & (SEG_HAS_ALPHA | SEG_REDUCED | SEG_ELEMWISE)):
        return "focal_fwd_lean_kernel<%d,%s>" % (_bucket(C, 4, 8), _b(ign))
    if what == SEG_FOCAL:
        return "focal_fwd_kernel<%d,%s,%s>" % (4 if vec else 1, _b(dense), _b(g2))
    if vec and C <= 16:
        share = labels and what != SEG_STATS and prob == PROB_SOFTMAX and not (f & SEG_ELEMWISE)
        plain = share and g2 and not cw and not (f & (SEG_HAS_IGNORE | SEG_HAS_ALPHA | SEG_REDUCED))
        so = what == SEG_STATS
        g = g2 or so
        assert not (share and (so or dense)) and not (so and not g) and not (plain and not (share and g)), case.name
        return "seg_loss_fwd_reg_kernel<4,16,%d,%s,%s,%s,%s>" % (2 if so else 3, _b(dense), _b(g), _b(share), _b(plain))
    return "seg_loss_fwd_kernel<%d>" % (4 if vec else 1)


def _smf(case, mode):
    """launch_smf<MODE>: every output (pixel map, gradient, upstream map) is a fresh allocation."""
    C, HW, g2 = case.C, case.HW, case.gamma == 2.0
    scalar, vec = bool(case.tun[0]), vec_ok(case)
    if mode == 0 and not scalar and HW % 256 == 0 and C <= 16 and g2 and not case.cw and case.threshold is None and vec:
        return "softmax_focal_lean_kernel<%d,0>" % _bucket(C, 4, 8, 16)
    if vec:
        if mode == 1 and C <= 16 and not scalar and case.tun[2]:
            return "softmax_focal_bwd_kernel<%d,16,%s,false>" % (case.tun[2], _b(g2))
        reg = C <= 16
        return "softmax_focal_kernel<4,%d,%d,%s>" % (16 if reg else 0, mode, _b(reg and g2))
    return "softmax_focal_kernel<1,0,%d,false>" % mode


def forward_arm(case):
    """The kernel instance the forward of a case launches.  "unsupported": ptb_region_loss_fwd serves the focal sums alone only from the
    packed kernel, FocalScalar.run() then returns None and nothing was launched.  RegionLoss outside the one-launch path:
    the streaming kernel + region_epilogue_kernel."""
    if case.family == "module":
        return forward_arm(routed(case))
    if case.family == "SoftmaxFocalSums":
        return _smf(case, 0)
    if case.family == "FocalScalar":
        return _seg_forward(case) if _focal_only_pk(case, SEG_FOCAL) else "unsupported"
    arm = _seg_forward(case)
    if case.family == "RegionLoss" and not case.one_launch:
        arm += "+region_epilogue_kernel"
    return arm


def _focal_bwd(case, gelem):
    return "focal_bwd_kernel<%d,%s,%s,%s>" % (4 if vec_ok(case) else 1, _b(case.target != "labels"), _b(gelem), _b(case.gamma == 2.0))


def _stats_bwd(case):
    """ptb_seg_stats_bwd."""
    dense, ign = case.target != "labels", case.ignore is not None
    if not case.tun[0] and dense and case.HW % 1024 == 0 and case.prob in (PROB_SIGMOID, PROB_IDENTITY) and case.HW % 4 == 0 and _aligned(case, "logits", "dense"):
        return "seg_dense_bwd_lean_kernel<%d,%s,false>" % (case.prob, _b(ign))
    if vec_ok(case):
        return "seg_stats_bwd_kernel<4,%d,false>" % (16 if case.C <= 16 and not dense else 0)
    return "seg_stats_bwd_kernel<1,0,false>"


def _fused_bwd(case):
    """ptb_seg_fused_bwd; PTB_EUNSUPPORTED: the Function launches the focal and the statistics backward and adds them."""
    f = flags_of(case)
    dense, labels, g2 = case.target != "labels", case.target == "labels", case.gamma == 2.0
    if (not case.tun[0] and dense and case.HW % 1024 == 0 and case.prob == PROB_SIGMOID and g2 and not case.cw and not (f & (SEG_HAS_ALPHA | SEG_REDUCED))
            and case.HW % 4 == 0 and _aligned(case, "logits", "dense")):
        return "seg_dense_bwd_lean_kernel<1,%s,true>" % _b(f & SEG_HAS_IGNORE)
    if case.C > 16 or not vec_ok(case) or (dense and case.prob == PROB_SOFTMAX):
        return _focal_bwd(case, False) + "+" + _stats_bwd(case)
    if labels and case.prob == PROB_SOFTMAX:
        plain = g2 and not case.cw and not (f & (SEG_HAS_IGNORE | SEG_HAS_ALPHA | SEG_REDUCED))
        if plain and case.HW % 256 == 0:
            return "seg_fused_bwd_lean_kernel<%d>" % _bucket(case.C, 4, 8, 16)
        return "seg_fused_bwd_shared_kernel<4,16,%s,%s>" % (_b(g2), _b(plain))
    return "seg_fused_bwd_kernel<4,16,%s,%s>" % (_b(dense), _b(g2))


def backward_arm(case):
    """The kernel instance(s) the backward of a case launches ("a+b": two launches and an add)."""
    if case.family == "module":
        return backward_arm(routed(case))
    if case.family == "SoftmaxFocalSums":
        return _smf(case, 1)
    if case.family in ("SigmoidFocalSums", "FocalScalar"):
        return _focal_bwd(case, case.elem)
    if case.family == "RegionStats" or (case.family == "RegionLoss" and not case.epi.with_focal):
        return _stats_bwd(case)
    return _fused_bwd(case)


def entry_points(case):
    """The C entry points the Function of a case calls, forward then backward, with the return code of each ("name:rc"); finalize /
    epilogue launches included.  The GPU file compares this with what the library was really asked."""
    fam, fwd, bwd = case.family, forward_arm(case), backward_arm(case)
    if fam == "module":
        r = routed(case)
        # BinaryFocalLoss() in its default configuration asks for the one-launch forward first
        declined = ["ptb_region_workspace_bytes", "ptb_region_loss_fwd:-2"] if _plain_binary_focal(case) and r.family != "FocalScalar" else []
        return declined + entry_points(r)
    if fam == "SoftmaxFocalSums":
        return ["ptb_softmax_focal_fwd:0", "ptb_sums_finalize:0", "ptb_softmax_focal_bwd:0"]
    if fam == "FocalScalar":
        if fwd == "unsupported":
            return ["ptb_region_workspace_bytes", "ptb_region_loss_fwd:-2"]
        return ["ptb_region_workspace_bytes", "ptb_region_loss_fwd:0", "ptb_focal_bwd:0"]
    if fam == "SigmoidFocalSums":
        return ["ptb_seg_loss_fwd:0", "ptb_sums_finalize:0", "ptb_focal_bwd:0"]
    if fam == "RegionStats":
        return ["ptb_seg_loss_fwd:0", "ptb_sums_finalize:0", "ptb_seg_stats_bwd:0"]
    fused = ["ptb_seg_fused_bwd:-2", "ptb_focal_bwd:0", "ptb_seg_stats_bwd:0"] if "+" in bwd else ["ptb_seg_fused_bwd:0"]
    if fam == "FusedSegSums":
        return ["ptb_seg_loss_fwd:0", "ptb_sums_finalize:0"] + fused
    head = ["ptb_region_workspace_bytes", "ptb_region_loss_fwd:0"] if case.one_launch else ["ptb_seg_loss_fwd:0", "ptb_region_epilogue:0"]
    return head + (fused if case.epi.with_focal else ["ptb_seg_stats_bwd:0"])


def forward_grid(case):
    """(wave-groups of work, workgroups launched) of the forward streaming kernel of a case: a wave takes one group per trip of its
    grid-stride loop, a workgroup has four waves, slot = workgroup % SUM_SLOTS."""
    arm = forward_arm(case)
    assert arm != "unsupported"
    B, C, HW = case.B, case.C, case.HW
    if arm.startswith("seg_focal_pk_kernel"):
        groups, cap = HW // 128 * B, GRID_FOCAL_PK
    elif arm.startswith("seg_stats_dense_lean_kernel"):
        groups, cap = HW // 1024 * C * B, GRID_STREAM
    elif arm.startswith(("seg_fwd_lean_kernel", "focal_fwd_lean_kernel", "softmax_focal_lean_kernel")):
        groups, cap = HW // 256 * B, GRID_STATS if arm.startswith("seg_fwd") else GRID_STREAM
    else:
        per = 256 if vec_ok(case) else 64
        groups = -(-HW // per) * B
        cap = GRID_STREAM if (case.family == "SoftmaxFocalSums" or what_of(case) == SEG_FOCAL) else GRID_STATS
    want = max(1, -(-groups // 4))
    return groups, min(want, case.tun[1] or cap)


def forward_trips(case):
    """(trips of the grid-stride loop, whether the last trip is partly filled)."""
    groups, grid = forward_grid(case)
    return -(-groups // (4 * grid)), groups % (4 * grid) != 0


# ------------------------------------------------------------------------------------------------- inputs
def numel(case):
    return case.B * case.C * case.HW


def n_extreme(case):
    """Extreme pixels of a case: four kinds of equal number at the start of image 0, at most one eighth of its pixels."""
    return case.HW // 8 // 4 * 4 if case.extreme else 0


def inputs(case):
    """dict(x, labels, dense, cw): float32 logits [B, C, HW] (probabilities in [0.01, 0.99] where the statistics take them as given),
    int64 labels [B, HW] or a float32 dense target [B, C, HW], float32 class weights [C] -- a function of the case only.

    Ignored elements: a run inside the first wave of image 0 and a wholly ignored wave (the first 256 pixels of the last image; with
    one image, pixels 256 .. 511); dense targets also 5 % of the elements at random and the first 1024 elements of the last plane.
    Extreme pixels (``n_extreme``), as test_softmax_focal_fast_and_exact_paths_agree_with_fp64 builds them: every class + 75, every
    class - 70, one class at -120 with the pixel's label on it, every class - 50 with the label's class another 70 below."""
    rng = np.random.default_rng(5000 + case.seed)
    B, C, HW = case.B, case.C, case.HW
    if case.prob == PROB_IDENTITY and case.family != "module":
        x = (rng.random((B, C, HW), dtype=np.float32) * np.float32(0.98) + np.float32(0.01)).astype(np.float32)
    else:
        # (dense targets under a softmax: the Jacobian's p_k (G_k - sum_c G_c p_c) cancels more, the logits are drawn narrower)
        x = (rng.standard_normal((B, C, HW)) * (2.0 if case.target != "labels" and case.prob == PROB_SOFTMAX else 2.5)).astype(np.float32)
    out = dict(x=x, labels=None, dense=None, cw=None)
    if case.cw:
        out["cw"] = (0.5 + 0.5 * (np.arange(C) % 3)).astype(np.float32)
    runs = [(0, min(5, HW - 1), min(21, HW))]
    if B >= 2:
        runs.append((B - 1, 0, min(HW, 256)))
    elif HW >= 512:
        runs.append((0, 256, 512))
    if case.target == "labels":
        if case.labels == "one":
            lab = np.full((B, HW), C // 2, dtype=np.int64)
        else:
            lab = rng.integers(0, max(C - 1, 1) if case.labels == "absent" else C, size=(B, HW)).astype(np.int64)
        n = n_extreme(case)
        if n:
            assert C >= 2 and case.prob != PROB_IDENTITY
            q = n // 4
            x[0, :, :q] += np.float32(75.0)
            x[0, :, q:2 * q] -= np.float32(70.0)
            x[0, 1, 2 * q:3 * q] = np.float32(-120.0)
            lab[0, 2 * q:3 * q] = 1
            x[0, :, 3 * q:n] -= np.float32(50.0)
            x[0, 0, 3 * q:n] -= np.float32(70.0)
            lab[0, 3 * q:n] = 0
        if case.ignored:
            for b, lo, hi in runs:
                lab[b, lo:hi] = case.ignore
        out["labels"] = lab
    else:
        assert not case.extreme
        u = rng.random((B, C, HW), dtype=np.float32)
        d = u if case.target == "soft" else (u < np.float32(0.3)).astype(np.float32)
        if case.ignored:
            d[rng.random((B, C, HW)) < 0.05] = case.ignore
            for b, lo, hi in runs:
                d[b, :, lo:hi] = case.ignore
            if B * C > 1:
                d[B - 1, C - 1, :min(HW, 1024)] = case.ignore
        out["dense"] = np.ascontiguousarray(d, dtype=np.float32)
    return out


def extreme_pixels(x):
    """[B, 1, HW] mask of the pixels whose gradients get the extreme tolerance: max_c |logit| > 60."""
    return np.abs(np.asarray(x)).max(axis=1, keepdims=True) > EXTREME_LOGIT


def bad_labels(case, inp):
    """The labels of a case with one label outside [0, C) that is not the ignore label (C itself, in the middle of image 0)."""
    lab = inp["labels"].copy()
    lab[0, case.HW // 2] = case.C if case.ignore != case.C else case.C + 1
    return lab


def epilogue_kwargs(case):
    e = case.epi
    mask = None
    if e.classes is not None:
        mask = np.zeros(case.C, dtype=np.uint8)
        mask[list(e.classes)] = 1
    return dict(focal_scale=(1.0 / numel(case)) if e.with_focal else 0.0, dice_weight=e.dice_weight, jaccard_weight=e.jaccard_weight, smooth=e.smooth,
                eps=e.eps, log_loss=e.log_loss, class_mask=mask, n_selected=case.C if e.classes is None else len(e.classes))


def _loss_scale(case, inp):
    """The upstream gradient of a scalar loss that brings the largest coefficient reaching the backward kernels to 1 (from the model)."""
    r = routed(case) if case.family == "module" else case
    if r.family == "RegionLoss":
        return 1.0 / np.abs(model(r, inp)["coef"]).max()
    if r.family == "SoftmaxFocalSums":
        return float(case.B * case.HW)
    if case.family == "module" and case.module[1].get("normalized"):
        return numel(case) * max(model(r._replace(family="SigmoidFocalSums"), inp)["focal"][1], 1e-6)
    return float(numel(case))


def upstream(case, inp=None):
    """Seeded unit-scale upstream coefficients, float32: one per sum ("focal" [2]; the second is 0 where the caller promises not to read
    the term sum), a vector for I and P ("stats" [3, C], the T row unused), a map for the element-wise / per-pixel output ("elem"), and
    for a scalar loss the factor that brings the coefficients reaching the backward kernels to unit scale ("loss")."""
    inp = inputs(case) if inp is None else inp
    rng = np.random.default_rng(9000 + case.seed)
    B, C, HW = case.B, case.C, case.HW
    up = dict(focal=(rng.random(2) + 0.5).astype(np.float32), stats=(rng.random((3, C)) + 0.5).astype(np.float32) * np.float32(rng.choice([-1.0, 1.0])),
              elem=(rng.random((B, C, HW) if case.family != "SoftmaxFocalSums" else (B, HW)) + 0.5).astype(np.float32),
              loss=np.float32(_loss_scale(case, inp) if case.family in ("RegionLoss", "FocalScalar", "module") else 1.0))
    if case.no_term:
        up["focal"][1] = 0.0
    up["stats"][2] = 0.0
    return up


def _focal_kw(case, cw):
    return dict(gamma=case.gamma, alpha=case.alpha, threshold=case.threshold, class_weights=cw, mask_term=case.mask_term)


def model(case, inp=None):
    """float64 model of everything the Function of a case returns: "focal" [2], "elem" (the element-wise or per-pixel map), "stats" [3, C],
    "loss" and "coef" [2 + 2C]."""
    inp = inputs(case) if inp is None else inp
    if case.family == "module":
        return module_model(case, inp)
    out = {}
    if case.family == "SoftmaxFocalSums":
        pix, sl, sf = SO.softmax_focal(inp["x"], inp["labels"], inp["cw"], case.gamma, case.threshold, case.ignore)
        out["focal"] = np.array([sl, sf])
        if case.elem:
            out["elem"] = pix
        return out
    t, ign = SO.targets(case.C, inp["labels"], inp["dense"], case.ignore)
    what = what_of(case)
    focal_sum = 0.0
    if what & SEG_FOCAL:
        L, sl, sf = SO.sigmoid_focal(inp["x"], t, ign, **_focal_kw(case, inp["cw"]))
        out["focal"], focal_sum = np.array([sl, sf]), sl
        if case.elem:
            out["elem"] = L
    if what & SEG_STATS:
        out["stats"] = np.stack(SO.region_stats(inp["x"], t, ign, case.prob))
    if case.family == "FocalScalar":
        return dict(loss=focal_sum / numel(case))
    if case.family == "RegionLoss":
        loss, coef = SO.region_epilogue(focal_sum, *out["stats"], **epilogue_kwargs(case))
        return dict(loss=loss, coef=coef)
    return out


def chain(case, dtype, inp=None):
    """(outputs, x): the reference's chain of a case in torch on the CPU, ``x`` the logits as a leaf that requires a gradient -- float64 for
    the gradient reference, float32 for the reference's own evaluation.  Same keys as ``model`` (without "coef")."""
    import torch

    inp = inputs(case) if inp is None else inp
    x = torch.from_numpy(inp["x"]).to(dtype).requires_grad_(True)
    cw = None if inp["cw"] is None else torch.from_numpy(inp["cw"])
    if case.family == "module":
        return module_chain(case, x, inp), x
    out = {}
    if case.family == "SoftmaxFocalSums":
        pix, f = SO.torch_softmax_focal(x, torch.from_numpy(inp["labels"]), cw, case.gamma, case.threshold, case.ignore)
        out["focal"] = torch.stack([pix.sum(), f.sum()])
        if case.elem:
            out["elem"] = pix
        return out, x
    t, ign = SO.torch_targets(case.C, inp["labels"], inp["dense"], case.ignore, dtype)
    what = what_of(case)
    focal_sum = None
    if what & SEG_FOCAL:
        L, F = SO.torch_sigmoid_focal(x, t, ign, **_focal_kw(case, cw))
        focal_sum = L.sum()
        out["focal"] = torch.stack([focal_sum, F.sum()])
        if case.elem:
            out["elem"] = L
    if what & SEG_STATS:
        out["stats"] = SO.torch_region_stats(x, t, ign, case.prob)
    if case.family == "FocalScalar":
        return dict(loss=focal_sum / numel(case)), x
    if case.family == "RegionLoss":
        return dict(loss=SO.torch_region_epilogue(focal_sum, out["stats"], **epilogue_kwargs(case))), x
    return out, x


def chain_gradient(case, dtype, inp=None, up=None):
    """(outputs as numpy, d sum(upstream * outputs) / d logits) of ``chain``."""
    import torch

    up = upstream(case, inp) if up is None else up
    out, x = chain(case, dtype, inp)
    total = sum((out[k] * torch.from_numpy(np.asarray(up[k])).to(dtype)).sum() for k in out)
    total.backward()
    return {k: v.detach().numpy() for k, v in out.items()}, x.grad.numpy()


def ratio(got, ref, rtol, atol, scale_atol=False):
    """Largest |got - ref| / (atol' + rtol |ref|) over ALL elements, atol' = atol * max(1, |ref|) for sums (as
    test_cfg4_scale_values_and_gradients_vs_torch scales it); NaN when a side is not finite."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    a = atol * np.maximum(1.0, np.abs(ref)) if scale_atol else atol
    err = np.abs(got - ref) / (a + rtol * np.abs(ref))
    return float("nan") if not np.isfinite(err).all() else float(err.max())


def gradient_ratio(got, ref, x):
    """The gradient comparison: tame pixels at GRAD_TOL, extreme pixels (decided from the logits) at GRAD_TOL_EXTREME; every element is
    in one of the two."""
    ext = np.broadcast_to(extreme_pixels(x), np.shape(ref))
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    r = ratio(got[~ext], ref[~ext], **GRAD_TOL)
    return max(r, ratio(got[ext], ref[ext], **GRAD_TOL_EXTREME)) if ext.any() else r


def value_ratios(case, got, want):
    """{key: worst error / tolerance} of the values of a case: T_c of hard labels and 0 / 1 targets exactly (inf when a count differs),
    the sums at TOL with atol scaled by max(1, |model|), maps, the scalar and its coefficients at TOL."""
    r = {}
    for k, w in want.items():
        g = np.asarray(got[k], dtype=np.float64)
        if k == "stats":
            r["I,P"] = ratio(g[:2], w[:2], scale_atol=True, **TOL)
            if case.target == "soft":
                r["T"] = ratio(g[2], w[2], scale_atol=True, **TOL)
            else:
                r["T"] = 0.0 if np.array_equal(g[2], w[2]) else float("inf")
        elif k == "focal":
            n = 1 if case.no_term else 2          # SEG_NO_TERM: the kernels may skip the term sum
            r[k] = ratio(g[:n], w[:n], scale_atol=True, **TOL)
        else:
            r[k] = ratio(g, w, **TOL)
    return r


# ------------------------------------------------------------------------------------------------- the module family
def _plain_binary_focal(case):
    """functional._sigmoid_focal: the configuration that tries FocalScalar before SigmoidFocalSums."""
    cls, kw = case.module
    return (cls == "BinaryFocalLoss" and case.target == "labels" and kw.get("reduction", "mean") in ("mean", "sum") and not kw.get("normalized")
            and kw.get("alpha") is None and kw.get("reduced_threshold") is None and kw.get("ignore_index") is None and kw.get("gamma", 2.0) == 2.0
            and kw.get("class_weights") is None)


def routed(case):
    """The Function-family case a public class must route to (losses/focal.py, dice.py, jaccard.py, fused.py through _region.py and
    functional.py): same tensors, the flags the Python layer sets."""
    cls, kw = case.module
    base = dict(B=case.B, C=case.C, HW=case.HW, target=case.target, off=case.off, t1=case.tun[0], t4=case.tun[1], t7=case.tun[2],
                t16=case.tun[3], t20=case.tun[4], labels=case.labels)
    if cls == "BinaryFocalLoss":
        plain = _plain_binary_focal(case)
        c = make_case("FocalScalar" if plain else "SigmoidFocalSums", gamma=kw.get("gamma", 2.0), alpha=kw.get("alpha"), threshold=kw.get("reduced_threshold"),
                      ignore=kw.get("ignore_index"), no_term=not kw.get("normalized"), mask_term=bool(kw.get("normalized")) and kw.get("ignore_index") is not None,
                      **base)
        if plain and forward_arm(c) == "unsupported":
            c = c._replace(family="SigmoidFocalSums")
        return c
    if cls == "CrossEntropyFocalLoss":
        return make_case("SoftmaxFocalSums", gamma=kw.get("gamma", 2.0), threshold=kw.get("reduced_threshold"), ignore=kw.get("ignore_index", -100),
                         ignored=case.ignored, **base)
    with_focal = cls == "FocalDiceJaccardLoss"
    epi = Epi(with_focal, kw.get("dice_weight", 0.0 if cls == "JaccardLoss" else 1.0), kw.get("jaccard_weight", 0.0 if cls == "DiceLoss" else 1.0),
              kw.get("smooth", 0.0), kw.get("eps", 1e-7), kw.get("log_loss", False), kw.get("classes"))
    prob = PROB_SOFTMAX if case.target == "labels" else PROB_SIGMOID
    return make_case("RegionLoss", prob=prob, gamma=kw.get("gamma", 2.0) if with_focal else 0.0, alpha=kw.get("alpha") if with_focal else None,
                     ignore=kw.get("ignore_index"), no_term=with_focal, epi=epi, **base)


def _module_shapes(case, inp):
    """The tensors as the public classes take them: logits [B, C, H, W] with H = 4, labels [B, H, W] or a dense target [B, C, H, W]."""
    H = 4
    assert case.HW % H == 0
    return (case.B, case.C, H, case.HW // H), (case.B, H, case.HW // H)


def module_model(case, inp):
    """The composed loss of a module case from oracle/losses_oracle.py."""
    from oracle import losses_oracle as LO

    cls, kw = case.module
    xs, ls = _module_shapes(case, inp)
    x = inp["x"].reshape(xs)
    y = inp["labels"].reshape(ls) if case.target == "labels" else inp["dense"].reshape(xs)
    mode = "multiclass" if case.target == "labels" else "multilabel"
    if cls == "BinaryFocalLoss":
        return dict(loss=LO.binary_focal_loss(x, y, **kw))
    if cls == "CrossEntropyFocalLoss":
        return dict(loss=LO.softmax_focal_loss_with_logits(x, y, **kw))
    if cls == "DiceLoss":
        return dict(loss=LO.dice_loss(x, y, mode, **kw))
    if cls == "JaccardLoss":
        return dict(loss=LO.jaccard_loss(x, y, mode, **kw))
    kw = dict(kw)
    wf, wd, wj = kw.pop("focal_weight", 1.0), kw.pop("dice_weight", 1.0), kw.pop("jaccard_weight", 1.0)
    fkw = dict(gamma=kw.pop("gamma", 2.0), alpha=kw.pop("alpha", None), ignore_index=kw.get("ignore_index"))
    focal = LO.binary_focal_loss(x, y, **fkw)
    jkw = {k: v for k, v in kw.items() if k != "ignore_index"}
    return dict(loss=wf * focal + wd * LO.dice_loss(x, y, mode, **kw) + wj * LO.jaccard_loss(x, y, mode, **jkw))


def module_chain(case, x, inp):
    """The module's loss in torch from the chains of oracle/seg_loss_oracle.py (the gradient reference of the module family)."""
    import torch

    cls, kw = case.module
    r = routed(case)
    if r.family == "SoftmaxFocalSums":
        pix, f = SO.torch_softmax_focal(x, torch.from_numpy(inp["labels"]), None, r.gamma, r.threshold, r.ignore)
        return dict(loss=pix.sum() / (case.B * case.HW))
    t, ign = SO.torch_targets(case.C, inp["labels"], inp["dense"], r.ignore, x.dtype)
    if r.family in ("SigmoidFocalSums", "FocalScalar"):
        L, F = SO.torch_sigmoid_focal(x, t, ign, **_focal_kw(r, None))
        total = L.sum() / F.sum().clamp_min(1e-6) if kw.get("normalized") else L.sum()
        return dict(loss=total / numel(case))
    focal_sum = None
    if r.epi.with_focal:
        focal_sum = SO.torch_sigmoid_focal(x, t, ign, **_focal_kw(r, None))[0].sum()
    ekw = epilogue_kwargs(r)
    ekw["focal_scale"] *= kw.get("focal_weight", 1.0)
    return dict(loss=SO.torch_region_epilogue(focal_sum, SO.torch_region_stats(x, t, ign, r.prob), **ekw))


# ------------------------------------------------------------------------------------------------- the tables
BUCKETS = ((3, 4), (4, 4), (5, 8), (8, 8), (9, 16), (16, 16))       # (C, register bucket): both sides of 4 / 8 / 16, C == bucket included
SHAPES_256 = ((1, 256), (2, 1024), (3, 1280), (1, 2048), (2, 256), (3, 1024))       # HW % 256 == 0


def _sigmoid_focal():
    cases, add = [], lambda *a, **kw: cases.append(make_case("SigmoidFocalSums", *a, **kw))
    for i, (C, _cr) in enumerate(BUCKETS):                       # the packed focal-only kernel: TERM x FULL x bucket
        for no_term in (False, True):
            add((1, 2, 3)[i % 3], C, (128, 384, 1280)[(i + no_term) % 3], no_term=no_term, extreme=(C, no_term) in ((16, False), (3, True)),
                labels=("rand", "absent", "one")[i % 3])
    # focal_fwd_lean_kernel<CCH, IGN>: the ignore label, tunable 20 off, C > 16 (class chunks of 8, the last one partly filled)
    for i, (C, kw) in enumerate(((4, dict(ignore=255)), (3, dict(t20=0)), (8, dict(ignore=255, mask_term=True)), (16, dict(t20=0)), (2, dict(ignore=255, no_term=True)),
                                 (17, dict()), (19, dict(ignore=255, mask_term=True)), (33, dict(no_term=True)), (1, dict(t20=0)), (9, dict(ignore=255)))):
        B, HW = SHAPES_256[i % len(SHAPES_256)]
        add(B, C, HW, **kw)
    # focal_fwd_kernel<PIX, DENSE, G2> / focal_bwd_kernel<PIX, DENSE, GELEM, G2>: the options crossed with the arms
    paths = (dict(HW=260), dict(HW=250), dict(HW=256, off=(1, 0, 0)), dict(HW=1024, off=(0, 1, 1)), dict(HW=1280, t1=1), dict(HW=60), dict(HW=4), dict(HW=252), dict(HW=1028), dict(HW=64))
    k = 0
    for target in ("labels", "dense", "soft"):
        for gamma in (2.0, 1.5, 0.0):
            for path in paths:
                for elem in (False, True):
                    if (k + elem) % 3 != 2 and path["HW"] not in (260, 250):         # a third of the remaining crossings is enough
                        k += 1
                        continue
                    rest = dict(path)
                    HW = rest.pop("HW")
                    ignore = (None, 255 if target == "labels" else (255.0, -100.0)[k % 2])[(k // 2) % 2]
                    add((1, 2, 3)[k % 3], (1, 2, 3, 5, 9, 17)[k % 6], HW, target=target, gamma=gamma, elem=elem, alpha=(None, 0.25, 0.75)[k % 3],
                        threshold=(None, 0.5)[(k // 3) % 2], cw=bool(k % 2), ignore=ignore, mask_term=ignore is not None and k % 4 < 2, **rest)
                    k += 1
    # hard labels, vector path, gamma 2 with ONE option each: what keeps a call off the straight-line kernels
    for kw in (dict(cw=True), dict(alpha=0.25), dict(threshold=0.5), dict(elem=True), dict(cw=True, elem=True, ignore=255)):
        add(2, 5, 1024, **kw)
    for t4 in (1, 3):                                            # several trips of the grid-stride loop, the last one partly filled
        add(3, 5, 1280, t4=t4)
        add(3, 5, 1280, t4=t4, ignore=255)
        add(2, 5, 1280, t4=t4, off=(1, 0, 0), alpha=0.25)
    return cases


def _focal_scalar():
    cases, add = [], lambda *a, **kw: cases.append(make_case("FocalScalar", *a, **kw))
    for i, (C, _cr) in enumerate(BUCKETS):
        add((1, 2, 3)[i % 3], C, (128, 384, 1280)[i % 3], no_term=bool(i % 2), extreme=C == 8)
    add(3, 4, 11008)                                             # 258 groups of 128 pixels: 65 workgroups, the slots wrap
    for t4 in (1, 3):
        add(3, 5, 1280, t4=t4, no_term=True)
    add(2, 5, 250, tag="unsupported")                            # what ptb_region_loss_fwd does not serve: nothing is launched
    add(2, 5, 1280, t4=3, off=(1, 0, 0), tag="unsupported")
    add(2, 5, 1280, off=(0, 1, 0), tag="unsupported")
    add(2, 5, 256, t20=0, tag="unsupported")
    add(2, 17, 256, tag="unsupported")
    return cases


def _region_stats():
    cases, add = [], lambda *a, **kw: cases.append(make_case("RegionStats", *a, **kw))
    for i, (prob, ignore) in enumerate(((PROB_SIGMOID, None), (PROB_SIGMOID, 255.0), (PROB_IDENTITY, None), (PROB_IDENTITY, -100.0))):
        add((3, 2)[i % 2], (3, 1, 5, 2)[i], (1024, 2048)[i % 2], target="dense" if i != 2 else "soft", prob=prob, ignore=ignore)      # the dense streaming kernels
    for i, (C, _cr) in enumerate(BUCKETS):
        B, HW = SHAPES_256[i]
        labels = ("rand", "absent", "one")[i % 3]
        add(B, C, HW, labels=labels, extreme=C == 9)                                    # the packed kernel, statistics alone
        add(B, C, HW, t20=0, labels=labels)                                              # seg_fwd_lean_kernel<CR, softmax, false>
        add(B, C, HW, ignore=255, t20=i % 2, extreme=C == 5)                             # <CR, softmax, true>
        add(B, C, HW, prob=PROB_IDENTITY, t20=i % 2)                                     # <CR, given, false>
        add(B, C, HW, prob=PROB_IDENTITY, ignore=255)                                    # <CR, given, true>
    k = 0
    for target in ("labels", "dense", "soft"):                  # the register-resident and the generic kernels
        for prob in (PROB_SOFTMAX, PROB_SIGMOID, PROB_IDENTITY):
            for path in (dict(HW=260), dict(HW=250), dict(HW=128), dict(HW=256, off=(1, 0, 0)), dict(HW=1024, off=(0, 1, 1)), dict(HW=1280, t1=1),
                         dict(HW=252, C=17), dict(HW=384, C=33), dict(HW=60), dict(HW=4), dict(HW=64, C=19), dict(HW=1028)):
                path = dict(path)
                HW, C = path.pop("HW"), path.pop("C", (1, 2, 3, 5, 9, 16)[k % 6])
                ignore = (None, 255 if target == "labels" else (255.0, -100.0)[k % 2])[(k // 2) % 2]
                if k % 2 == 0 or HW == 260:
                    add((1, 2, 3)[k % 3], C, HW, target=target, prob=prob, ignore=ignore, **path)
                k += 1
    add(2, 5, 1024, prob=PROB_SIGMOID)                           # hard labels with a sigmoid: no straight-line kernel
    add(2, 5, 1024, prob=PROB_SIGMOID, ignore=255)
    for target, prob in (("labels", PROB_SOFTMAX), ("dense", PROB_SIGMOID), ("soft", PROB_SOFTMAX)):      # tunable 1: the scalar kernels on a vector shape
        add(2, 5, 1280, t1=1, target=target, prob=prob, ignore=-100.0 if target == "soft" else None)
    for t4 in (1, 3):
        add(3, 5, 1280, t4=t4)
        add(3, 5, 1280, t4=t4, t20=0, ignore=255)
        add(3, 5, 1024, t4=t4, target="dense", prob=PROB_SIGMOID)
        add(2, 5, 1280, t4=t4, off=(1, 0, 0))
    return cases


def _softmax_focal():
    cases = []

    def add(*a, **kw):
        kw.setdefault("ignore", -100)
        kw.setdefault("ignored", len(cases) % 2 == 0)
        cases.append(make_case("SoftmaxFocalSums", *a, **kw))

    for i, (C, _cr) in enumerate(BUCKETS):                       # the straight-line forward; every backward variant (tunable 7)
        B, HW = SHAPES_256[i]
        add(B, C, HW, t7=(4, 2, 0)[i % 3], elem=bool(i % 2), extreme=C in (4, 9, 16), labels=("rand", "absent", "one")[i % 3])
    k = 0
    for gamma in (2.0, 1.5, 0.0):                                # softmax_focal_kernel<PIX, CREG, MODE, G2>, softmax_focal_bwd_kernel<PIX, 16, G2, false>
        for path in (dict(HW=260), dict(HW=250), dict(HW=256, cw=True), dict(HW=1024, threshold=0.5), dict(HW=256, off=(1, 0, 0)), dict(HW=1024, off=(0, 1, 0)),
                     dict(HW=1280, t1=1), dict(HW=252, C=17), dict(HW=384, C=33), dict(HW=60), dict(HW=4), dict(HW=64, C=19, cw=True), dict(HW=128, threshold=0.3, cw=True), dict(HW=1028)):
            path = dict(path)
            HW, C = path.pop("HW"), path.pop("C", (2, 3, 5, 9, 16, 1)[k % 6])
            add((1, 2, 3)[k % 3], C, HW, gamma=gamma, t7=(4, 2, 0)[k % 3], elem=bool(k % 2), **path)
            k += 1
    for t7 in (4, 2, 0):                                         # tame and extreme pixels in the exact paths of each backward
        add(2, 16, 1024, t7=t7, extreme=True, ignored=True)
        add(2, 5, 260, t7=t7, extreme=True, gamma=1.5, elem=True)
    add(2, 17, 256, extreme=True)
    for t4 in (1, 3):
        add(3, 5, 1280, t4=t4)
        add(3, 5, 1280, t4=t4, gamma=1.5, t7=0, elem=True)
        add(2, 5, 1280, t4=t4, off=(1, 0, 0))
    return cases


def _fused():
    cases, add = [], lambda *a, **kw: cases.append(make_case("FusedSegSums", *a, **kw))
    for i, ignore in enumerate((None, 255.0, -100.0)):           # dense targets, the streaming kernels
        add((3, 2, 1)[i], (3, 1, 5)[i], (1024, 2048, 1024)[i], target=("dense", "dense", "soft")[i], prob=PROB_SIGMOID, ignore=ignore, mask_term=i == 1)
    for i, (C, cr) in enumerate(BUCKETS):                        # the packed kernel (TERM, FULL) and the straight-line backward
        B, HW = SHAPES_256[i]
        labels = ("rand", "absent", "one")[i % 3]
        add(B, C, HW, no_term=True, t16=i % 2, labels=labels, extreme=C in (3, 16))
        add(B, C, HW, no_term=False, t16=(i + 1) % 2, extreme=C in (8, 9))
    k = 0
    for target in ("labels", "dense", "soft"):                   # the register-resident / generic forward, the shared / generic / split backward
        for prob in (PROB_SOFTMAX, PROB_SIGMOID, PROB_IDENTITY):
            for gamma in (2.0, 1.5, 0.0):
                for path in (dict(HW=260), dict(HW=1024, cw=True), dict(HW=256, alpha=0.25), dict(HW=1280, threshold=0.5), dict(HW=250), dict(HW=256, off=(1, 0, 0)),
                             dict(HW=1024, off=(0, 1, 1)), dict(HW=1280, t1=1), dict(HW=252, C=17), dict(HW=128), dict(HW=60), dict(HW=4), dict(HW=1028), dict(HW=64), dict(HW=384, C=19)):
                    k += 1
                    if not ((path["HW"] == 260 and gamma == 2.0) or k % 4 == 0):
                        continue
                    path = dict(path)
                    HW, C = path.pop("HW"), path.pop("C", (2, 3, 5, 9, 16, 1)[k % 6])
                    ignore = (None, 255 if target == "labels" else (255.0, -100.0)[k % 2])[(k // 2) % 2]
                    add((1, 2, 3)[k % 3], C, HW, target=target, prob=prob, gamma=gamma, ignore=ignore, mask_term=ignore is not None and k % 4 < 2,
                        no_term=k % 5 == 0, **path)
    for kw in (dict(HW=260), dict(HW=1024, ignore=255), dict(HW=1024, gamma=1.5), dict(HW=1024, cw=True, alpha=0.75), dict(HW=260, threshold=0.5, gamma=0.0)):
        add(2, kw.pop("C", 9), kw.pop("HW"), extreme=True, **kw)     # the redo paths of the shared-exponent kernels
    for t4 in (1, 3):
        add(3, 5, 1280, t4=t4)
        add(3, 5, 1280, t4=t4, ignore=255)
        add(3, 5, 1024, t4=t4, target="dense", prob=PROB_SIGMOID)
        add(2, 5, 1280, t4=t4, off=(1, 0, 0))
    return cases


def _region_loss():
    cases, add = [], lambda *a, **kw: cases.append(make_case("RegionLoss", *a, **kw))
    epis = (Epi(False, 1.0, 0.0, 0.0, 1e-7, False, None), Epi(False, 0.0, 1.0, 1.0, 1e-7, True, None), Epi(True, 0.7, 1.3, 0.0, 1e-7, False, None),
            Epi(True, 1.0, 1.0, 1.0, 1e-7, True, None), Epi(False, 1.0, 0.5, 0.5, 1e-7, True, (0, 2)), Epi(True, 0.5, 0.0, 0.0, 1e-7, False, (1, 2)))
    k = 0
    for one_launch in (True, False):                             # the in-launch tail and the epilogue kernel behind every kind of streaming kernel
        for kw in (dict(HW=1280), dict(HW=256, t20=0), dict(HW=1024, ignore=255), dict(HW=1024, prob=PROB_IDENTITY), dict(HW=260), dict(HW=250), dict(HW=252, C=17),
                   dict(HW=1024, target="dense", prob=PROB_SIGMOID), dict(HW=2048, target="dense", prob=PROB_SIGMOID, ignore=255.0), dict(HW=384, target="soft", prob=PROB_IDENTITY),
                   dict(HW=256, off=(1, 0, 0)), dict(HW=1280, t1=1), dict(HW=1024, labels="absent"), dict(HW=1024, extreme=True), dict(HW=128, gamma=1.5), dict(HW=60, alpha=0.25)):
            for j in (0, 1):
                kw2 = dict(kw)
                epi = epis[(k + 3 * j) % len(epis)]
                if not epi.with_focal:
                    for name in ("gamma", "alpha"):
                        kw2.pop(name, None)
                    kw2["gamma"] = 0.0
                C = kw2.pop("C", (3, 5, 9, 16)[k % 4])
                add((1, 2, 3)[k % 3], C, kw2.pop("HW"), epi=epi, one_launch=one_launch, no_term=epi.with_focal, **kw2)
            k += 1
    add(3, 4, 11008, epi=epis[2], no_term=True)                  # the slots wrap under the tail
    for t4 in (1, 3):
        add(3, 5, 1280, t4=t4, epi=epis[2], no_term=True)
        add(3, 5, 1280, t4=t4, epi=epis[0], t20=0, gamma=0.0)
        add(2, 5, 1280, t4=t4, epi=epis[3], no_term=True, off=(1, 0, 0))
    return cases


def _modules():
    cases = []

    def add(cls, kw, B, C, HW, **ckw):
        cases.append(make_case("module", B, C, HW, module=(cls, kw), **ckw))

    add("BinaryFocalLoss", dict(), 2, 5, 1280)
    add("BinaryFocalLoss", dict(), 2, 5, 252)
    add("BinaryFocalLoss", dict(alpha=0.25, gamma=1.5, ignore_index=255, normalized=True), 2, 5, 1024, ignore=255)
    add("BinaryFocalLoss", dict(reduced_threshold=0.5), 2, 3, 260, target="dense")
    add("CrossEntropyFocalLoss", dict(), 2, 5, 1024, ignore=-100)
    add("CrossEntropyFocalLoss", dict(gamma=1.5, reduced_threshold=0.5), 2, 17, 252, ignore=-100, ignored=False)
    add("DiceLoss", dict(), 2, 5, 1280)
    add("DiceLoss", dict(log_loss=True, smooth=1.0, ignore_index=255, classes=[0, 2]), 2, 5, 1024, ignore=255)
    add("DiceLoss", dict(), 2, 3, 1024, target="dense")
    add("JaccardLoss", dict(), 2, 9, 1024)
    add("JaccardLoss", dict(log_loss=True, smooth=1.0), 2, 17, 252)
    add("FocalDiceJaccardLoss", dict(), 2, 16, 1024)
    add("FocalDiceJaccardLoss", dict(alpha=0.25, gamma=1.5, dice_weight=0.5, jaccard_weight=2.0), 2, 5, 260)
    add("FocalDiceJaccardLoss", dict(), 2, 3, 1024, target="dense")
    return cases


SIGMOID_FOCAL, FOCAL_SCALAR, REGION_STATS, SOFTMAX_FOCAL, FUSED, REGION_LOSS, MODULES = (
    _sigmoid_focal(), _focal_scalar(), _region_stats(), _softmax_focal(), _fused(), _region_loss(), _modules())
FUNCTIONS = SIGMOID_FOCAL + FOCAL_SCALAR + REGION_STATS + SOFTMAX_FOCAL + FUSED + REGION_LOSS
ALL = FUNCTIONS + MODULES
ids = lambda c: c.name  # noqa: E731


def bad_label_cases():
    """One case per forward arm that reads hard labels (the first of the tables that reaches it)."""
    seen, out = set(), []
    for case in FUNCTIONS:
        arm = forward_arm(case)
        if case.target == "labels" and arm != "unsupported" and arm not in seen:
            seen.add(arm)
            out.append(case)
    return out


# Kernel instances of ptb_losses.hip that no case reaches, each with its reason (tests/test_seg_loss_sweep_cpu.py fails on an instance
# that is neither reached nor listed here, and on an entry that a case does reach).
UNREACHED = {}
