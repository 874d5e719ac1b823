"""Cases and a float64 model of the hard-example-mining losses (losses/hard_mining.py): value, threshold, kept count and gradient.

THE MODEL restates the definitions, nothing of the implementation: the element losses from torch's float64 ``cross_entropy`` /
``binary_cross_entropy_with_logits`` with ``reduction="none"`` on the float32 logits widened, then numpy: the elements that are not
ignored form the selection sets, ``kept`` follows the top-k or OHEM rule, ``thr`` is the ``kept``-th largest loss, the loss is
``(sum_{l > thr} l + (kept - gt) thr) / kept``, the ``eq`` elements at ``thr`` weigh ``(kept - gt) / eq``, and the gradient is
``coef * weight / kept * (p - target)`` for a seeded unit-scale upstream coefficient per result.  Two float64 losses count as equal within
1e-12 relative: bit-identical logit vectors must tie whatever path torch's vectorised kernels take for them.

THE CASES are the smallest that reach every path of csrc/ptb_hard_mining.hip: S of 5, 1023, 1027 and 3077 (peeled; below / above one
workgroup's 1024 positions; several partial-sum slots) and 1024, 4096 and a volume (16-byte accesses); every channel handling at and just
over its edge (softmax buckets 4 / 8 / 16, the sweep above them, independent sigmoid channels); B of 1 and 3; both ``per_sample``; k from
100 % down to a single kept element; logit scales 1 and 4 and positions at +-60; ignored elements scattered, a whole sample and
everything; OHEM in either branch, with the count above ``t0`` equal to ``min_kept``, with nothing kept and with ``min_kept > n``; and
ties: all vectors identical, and two groups of identical vectors with the cut inside either.

NEAR-CUT ELEMENTS: the device rounds element losses to fp32, the model does not.  An element whose float64 loss lies within
``TOL["rtol"] * max(1, thr)`` of the model's ``thr`` is UNDECIDED: ``check`` accepts for it the kept or the unkept model gradient.  Every
other element has one model gradient, and the kept count must match exactly.  ``undecided`` is a property of the model alone, and the
seeds keep it at 3 elements at most per set in every tie-free case (tests/test_hard_mining_cpu.py asserts it)."""
import functools
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import seg_loss_cases as SC

IGNORE = 255
EXTREME_LOGIT = 60.0
EQ64 = 1e-12                 # relative width of "equal" between float64 element losses
SHAPES = {5: (1, 5), 1023: (31, 33), 1024: (32, 32), 1027: (13, 79), 3077: (17, 181), 4096: (64, 64), 660: (6, 10, 11)}


class Case(NamedTuple):
    name: str
    mode: str = "multiclass"
    B: int = 1
    C: int = 3
    S: int = 1027
    rule: str = "topk"
    k: float = 10.0
    thresh: float = 0.7
    min_kept: object = 0             # an int, or "above": the number of losses above t0 of the (first) set
    per_sample: bool = False
    reduction: str = "mean"
    ignore: Optional[str] = None     # scatter (30 % of the elements) | sample (sample 1 entirely) | all
    scale: float = 1.0
    extreme: bool = False            # logits of +-60 at a few positions
    pattern: str = "random"          # random | identical | groups (two groups of identical vectors, 30 % in the harder one)
    seed: int = 0

    @property
    def spatial(self) -> Tuple[int, ...]:
        return SHAPES[self.S]

    @property
    def ties(self) -> bool:
        return self.pattern != "random"


def _cases():
    c = []
    for S in (5, 1023, 1024, 1027, 3077, 4096, 660):
        B = 2 if S == 660 else 3
        c.append(Case(f"s{S}", B=B, S=S))
        c.append(Case(f"s{S}_per_sample", B=B, S=S, per_sample=True, reduction="none"))
    for C in (2, 4, 5, 8, 9, 16, 17, 19):
        c.append(Case(f"c{C}", C=C, k=50.0))
    for C in (4, 8, 16, 17):
        c.append(Case(f"c{C}_wide", C=C, S=1024, k=50.0, B=3, per_sample=True))
    for S in (1027, 1024):
        c.append(Case(f"binary_s{S}", mode="binary", C=1, S=S, B=3))
        c.append(Case(f"multilabel_s{S}", mode="multilabel", C=3, S=S, B=1, k=50.0))
    c.append(Case("multilabel_per_sample", mode="multilabel", C=3, S=1027, B=3, per_sample=True, reduction="none"))
    c.append(Case("multilabel_volume", mode="multilabel", C=3, S=660, B=2, k=1.0))
    for k, tag in ((100.0, "100"), (50.0, "50"), (10.0, "10"), (1.0, "1"), (1e-3, "one")):
        c.append(Case(f"k{tag}", B=3, C=5, S=3077, k=k))
        c.append(Case(f"k{tag}_per_sample", B=3, C=5, S=3077, k=k, per_sample=True))
    c += [Case("scale4", C=5, scale=4.0), Case("scale4_c17", C=17, scale=4.0, k=1.0), Case("extreme", C=5, extreme=True, k=1.0),
          Case("extreme_c19", C=19, extreme=True, B=3, per_sample=True, reduction="none"),
          Case("extreme_binary", mode="binary", C=1, extreme=True, scale=4.0)]
    c += [Case("ignore", B=3, ignore="scatter"), Case("ignore_wide", B=3, C=9, S=1024, ignore="scatter", per_sample=True, reduction="none"),
          Case("ignore_binary", mode="binary", C=1, B=3, ignore="scatter"),
          Case("ignore_multilabel", mode="multilabel", C=3, S=1024, ignore="scatter", per_sample=True),
          Case("ignore_sample", B=3, ignore="sample"), Case("ignore_sample_per_sample", B=3, ignore="sample", per_sample=True, reduction="none"),
          Case("ignore_sample_mean", B=3, C=17, ignore="sample", per_sample=True),
          Case("ignore_all", B=3, ignore="all"), Case("ignore_all_per_sample", B=3, ignore="all", per_sample=True, reduction="none"),
          Case("ignore_all_multilabel", mode="multilabel", C=3, B=1, S=5, ignore="all")]
    # OHEM: t0 = -log(thresh); random labels on C = 5 unit-scale logits leave most losses above -log(0.7) = 0.36, few above -log(0.02) = 3.9
    c += [Case("ohem_above", rule="ohem", B=3, C=5, thresh=0.7, min_kept=100),
          Case("ohem_floor", rule="ohem", B=3, C=5, thresh=0.02, min_kept=700),
          Case("ohem_equal", rule="ohem", B=3, C=5, thresh=0.3, min_kept="above"),
          Case("ohem_nothing", rule="ohem", B=3, C=5, thresh=1e-30, min_kept=0),
          Case("ohem_everything", rule="ohem", B=3, C=5, thresh=0.02, min_kept=10 ** 6),
          Case("ohem_per_sample", rule="ohem", B=3, C=17, S=3077, thresh=0.02, min_kept=400, per_sample=True, reduction="none"),
          Case("ohem_per_sample_above", rule="ohem", B=3, C=4, S=1024, thresh=0.5, min_kept=50, per_sample=True),
          Case("ohem_ignore", rule="ohem", B=3, C=8, thresh=0.7, min_kept=100, ignore="scatter"),
          Case("ohem_ignore_sample", rule="ohem", B=3, C=5, thresh=0.02, min_kept=300, ignore="sample", per_sample=True, reduction="none"),
          Case("ohem_binary", rule="ohem", mode="binary", C=1, B=3, thresh=0.7, min_kept=100),
          Case("ohem_multilabel_floor", rule="ohem", mode="multilabel", C=3, S=1024, thresh=0.01, min_kept=900)]
    c += [Case("tie_identical", C=4, pattern="identical"), Case("tie_identical_per_sample", B=3, C=5, S=1024, pattern="identical", per_sample=True,
                                                                reduction="none"),
          Case("tie_identical_binary", mode="binary", C=1, pattern="identical", k=50.0),
          Case("tie_groups_hard", C=4, pattern="groups", k=10.0), Case("tie_groups_easy", C=4, pattern="groups", k=50.0),
          Case("tie_groups_c17", C=17, S=3077, B=3, pattern="groups", k=50.0, per_sample=True, reduction="none"),
          Case("tie_groups_multilabel", mode="multilabel", C=3, S=1024, pattern="groups", k=50.0),
          Case("tie_ohem_floor", rule="ohem", C=4, pattern="groups", thresh=0.001, min_kept=100)]
    return {k.name: k for k in c}


CASES = _cases()
TIE_CASES = tuple(n for n, k in CASES.items() if k.ties)
TIE_FREE = tuple(n for n, k in CASES.items() if not k.ties)


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def inputs(name):
    """``(x float32 [B, C, *spatial], target)``: int64 labels ``[B, *spatial]`` (multiclass) or float32 targets in [0, 1] of the logits' shape"""
    case = CASES[name]
    rng = np.random.default_rng(7000 + sum((i + 1) * ord(ch) for i, ch in enumerate(name)) + case.seed)
    B, C, S = case.B, case.C, case.S
    dense = case.mode != "multiclass"
    if case.pattern == "random":
        x = rng.normal(0.0, case.scale, (B, C, S))
        t = rng.random((B, C, S)).round(2) if dense else rng.integers(0, C, (B, S))      # soft targets: the loss takes any g in [0, 1]
    else:
        vectors = rng.normal(0.0, 1.5, (2, C))
        group = (rng.random((B, S)) < 0.3).astype(np.int64) if case.pattern == "groups" else np.zeros((B, S), np.int64)
        x = np.moveaxis(vectors[group], -1, 1)                                            # [B, C, S]
        targets = (rng.random((2, C)) < 0.5).astype(np.float64) if dense else rng.integers(0, C, 2)
        if not dense:                                                                      # vector 1, the 30 %, is the harder one
            ce = [np.log(np.exp(v).sum()) - v[y] for v, y in zip(vectors, targets)]
            if ce[1] < ce[0]:
                vectors, targets = vectors[::-1], targets[::-1]
        t = np.moveaxis(targets[group], -1, 1) if dense else targets[group]
    if case.extreme:
        for i, p in enumerate(rng.choice(S, 6, replace=False)):
            x[i % B, rng.integers(C), p] = EXTREME_LOGIT if i % 2 else -EXTREME_LOGIT
    x = x.astype(np.float32).reshape((B, C) + case.spatial)
    t = t.astype(np.float32 if dense else np.int64)
    if case.ignore == "scatter":
        t[rng.random(t.shape) < 0.3] = IGNORE
    elif case.ignore == "sample":
        t[1] = IGNORE
    elif case.ignore == "all":
        t[...] = IGNORE
    t = t.reshape(((B, C) if dense else (B,)) + case.spatial)
    x.setflags(write=False)
    t.setflags(write=False)
    return x, t


def arguments(case):
    """keyword arguments of ``topk_cross_entropy`` / ``ohem_cross_entropy`` (and, without ``mode`` moved, of the modules)"""
    kw = dict(mode=case.mode, ignore_index=IGNORE if case.ignore else None, per_sample=case.per_sample, reduction=case.reduction)
    if case.rule == "topk":
        kw["k"] = case.k
    else:
        kw["thresh"] = case.thresh
        kw["min_kept"] = min_kept(case.name)
    return kw


def t0_of(case):
    return float(np.float32(-math.log(case.thresh)))


# ---------------------------------------------------------------------------------------------------------------- the model
class Model(NamedTuple):
    loss: np.ndarray             # float64 [] or [B] (before the mean over samples of reduction="mean")
    thr: np.ndarray              # float64, inf for an empty kept set
    kept: np.ndarray             # int64
    coef: np.ndarray             # float64 [sets]: the upstream gradient of every result
    grad: np.ndarray             # float64 [B, C, *spatial]: of (loss * coef).sum()
    grad_flipped: np.ndarray     # the same with every UNDECIDED element's weight flipped between kept (1) and unkept (0)
    undecided: np.ndarray        # bool [B, C, *spatial] (multiclass: the same for every channel of a position)
    undecided_per_set: np.ndarray
    near_t0: int                 # OHEM: elements within the near-cut width of t0 (the seeds keep it at 0)
    weight: np.ndarray           # float64 [B, E] element weights
    scale: np.ndarray            # float64 [B, 1...]: |coef| / kept of the element's set, the unit of the gradient's absolute bound


@functools.lru_cache(maxsize=None)
def _elements(name):
    """float64 element losses ``[B, E]``, validity, and d loss / d logits ``[B, C, *spatial]``"""
    case = CASES[name]
    x, t = inputs(name)
    xt = torch.from_numpy(x.copy()).double()
    valid = t != IGNORE
    if case.mode == "multiclass":
        lab = torch.from_numpy(np.where(valid, t, 0))
        l = F.cross_entropy(xt, lab, reduction="none").numpy()
        d = torch.softmax(xt, dim=1).numpy()
        d = d - np.moveaxis(np.eye(case.C)[lab.numpy()], -1, 1)
    else:
        g = torch.from_numpy(np.where(valid, t, 0.0)).double()
        l = F.binary_cross_entropy_with_logits(xt, g, reduction="none").numpy()
        d = torch.sigmoid(xt).numpy() - g.numpy()
    return l.reshape(case.B, -1), valid.reshape(case.B, -1), d


def _kept(case, n, above, floor):
    if n == 0:
        return 0
    if case.rule == "topk":
        return min(n, max(1, int(math.floor(np.float64(n) * case.k / 100))))
    m = min(floor, n)
    return above if above >= m else m


@functools.lru_cache(maxsize=None)
def min_kept(name):
    case = CASES[name]
    if case.min_kept != "above":
        return int(case.min_kept)
    l, valid, _ = _elements(name)
    sel = slice(0, 1) if case.per_sample else slice(None)
    return int((l[sel][valid[sel]] > t0_of(case)).sum())


@functools.lru_cache(maxsize=None)
def model(name):
    case = CASES[name]
    l, valid, d = _elements(name)
    B, E = l.shape
    sets = B if case.per_sample else 1
    ls, vs = l.reshape(sets, -1), valid.reshape(sets, -1)
    rng = np.random.default_rng(99 + sum(map(ord, name)))
    coef = rng.uniform(0.5, 1.5, sets) * rng.choice([-1.0, 1.0], sets)
    if case.per_sample and case.reduction == "mean":
        coef = np.full(sets, coef[0])
    loss, thr, kept = np.zeros(sets), np.full(sets, np.inf), np.zeros(sets, np.int64)
    weight, flipped, undecided = np.zeros(ls.shape), np.zeros(ls.shape), np.zeros(ls.shape, bool)
    near_t0 = 0
    t0 = t0_of(case) if case.rule == "ohem" else 0.0
    for s in range(sets):
        v = ls[s][vs[s]]
        n = v.size
        above = int((v > t0).sum())
        kept[s] = _kept(case, n, above, min_kept(name) if case.rule == "ohem" else 0)
        if case.rule == "ohem":
            near_t0 += int((np.abs(v - t0) <= SC.TOL["rtol"] * max(1.0, t0)).sum())
        if kept[s] == 0:
            continue
        th = np.sort(v)[n - kept[s]]
        eq = vs[s] & (np.abs(ls[s] - th) <= EQ64 * max(1.0, th))
        gt = vs[s] & (ls[s] > th) & ~eq
        thr[s] = th
        tied = kept[s] - gt.sum()
        assert 1 <= tied <= eq.sum(), (name, s, kept[s], gt.sum(), eq.sum())
        loss[s] = (ls[s][gt].sum() + tied * th) / kept[s]
        weight[s] = gt + eq * (tied / eq.sum())
        undecided[s] = vs[s] & (np.abs(ls[s] - th) <= SC.TOL["rtol"] * max(1.0, th))
        flipped[s] = np.where(undecided[s], np.where(weight[s] > 0.5, 0.0, 1.0), weight[s])
    unit = coef / np.maximum(kept, 1)
    if case.per_sample and case.reduction == "mean":
        unit = unit / sets

    def gradient(w):
        per_element = (w * unit[:, None]).reshape(B, E)
        per_element = per_element.reshape((B, 1) + d.shape[2:]) if case.mode == "multiclass" else per_element.reshape(d.shape)
        return per_element * d

    und = undecided.reshape(B, E)
    und = np.broadcast_to(und.reshape((B, 1) + d.shape[2:]), d.shape) if case.mode == "multiclass" else und.reshape(d.shape)
    scale = np.abs(np.broadcast_to(unit[:, None], ls.shape).reshape(B, E)[:, :1]).reshape((B,) + (1,) * (d.ndim - 1))
    if not case.per_sample:
        loss, thr, kept_out = loss.reshape(()), thr.reshape(()), kept.reshape(())
    else:
        kept_out = kept
    return Model(loss, thr, kept_out, coef, gradient(weight), gradient(flipped), und, undecided.sum(axis=1), near_t0, weight.reshape(B, E), scale)


# ---------------------------------------------------------------------------------------------------------------- calls and checks
def run(name, fn_topk, fn_ohem, device=None, x=None, t=None, **extra):
    """Calls the loss of a case with ``return_threshold=True`` and backpropagates ``(loss * coef).sum()``; returns detached
    ``(loss, thr, kept, grad)`` on the device they were computed on.  ``x`` / ``t``: tensors instead of the case's inputs."""
    case = CASES[name]
    x0, t0 = inputs(name)
    xt = (torch.from_numpy(x0.copy()) if x is None else x.detach().clone())
    tt = torch.from_numpy(t0.copy()) if t is None else t
    if device is not None:
        xt, tt = xt.to(device), tt.to(device)
    xt.requires_grad_(True)
    kw = arguments(case)
    kw.update(extra)
    loss, thr, kept = (fn_topk if case.rule == "topk" else fn_ohem)(xt, tt, return_threshold=True, **kw)
    coef = torch.from_numpy(model(name).coef).to(loss.device, torch.float32)
    (loss * (coef[0] if loss.dim() == 0 else coef)).sum().backward()
    return loss.detach(), thr.detach(), kept.detach(), xt.grad.detach()


def check(name, loss, thr, kept, grad, verbose=True):
    """loss and thr within ``seg_loss_cases.TOL`` of the model, the kept count exactly, the gradient within ``GRAD_TOL`` -- its absolute
    part in units of |coef| / kept, the size of a kept element's d loss / d logit = p - target, which is what fp32 rounds at unit scale.
    In the tie-free cases an undecided element may have the gradient of either decision; in the tie cases nothing is undecided."""
    case = CASES[name]
    want = model(name)
    got_loss, got_thr = loss.cpu().numpy().astype(np.float64), thr.cpu().numpy().astype(np.float64)
    want_loss = want.loss.mean() if case.per_sample and case.reduction == "mean" else want.loss
    assert loss.dtype == torch.float32 and thr.dtype == torch.float32 and kept.dtype == torch.int64
    assert got_loss.shape == np.shape(want_loss) and got_thr.shape == want.thr.shape and tuple(kept.shape) == want.kept.shape
    assert np.array_equal(kept.cpu().numpy(), want.kept), (name, kept.cpu().numpy(), want.kept)
    err = np.abs(got_loss - want_loss)
    bound = SC.TOL["rtol"] * np.abs(want_loss) + SC.TOL["atol"]
    if verbose:
        print(f"{name}: loss {got_loss} model {want_loss} err {np.max(err):.3e} bound {np.min(bound):.3e}; thr {got_thr} model {want.thr}; kept {want.kept}")
    assert (err <= bound).all(), (name, got_loss, want_loss)
    finite = np.isfinite(want.thr)
    assert np.array_equal(np.isposinf(got_thr), ~finite), (name, got_thr, want.thr)
    thr_err = np.abs(np.where(finite, got_thr, 0.0) - np.where(finite, want.thr, 0.0))
    assert (thr_err <= SC.TOL["rtol"] * np.where(finite, np.abs(want.thr), 0.0) + SC.TOL["atol"]).all(), (name, got_thr, want.thr)
    g = grad.cpu().numpy().astype(np.float64)
    assert g.shape == want.grad.shape

    def within(model_grad):
        return np.abs(g - model_grad) <= SC.GRAD_TOL["rtol"] * np.abs(model_grad) + SC.GRAD_TOL["atol"] * want.scale

    ok = within(want.grad)
    if not case.ties:
        either = within(want.grad_flipped)
        if case.mode == "multiclass":                      # a position is decided once: all its channels follow the same decision
            either = np.broadcast_to(either.all(axis=1, keepdims=True), ok.shape)
            ok = np.where(want.undecided, np.broadcast_to(ok.all(axis=1, keepdims=True), ok.shape) | either, ok)
        else:
            ok = np.where(want.undecided, ok | either, ok)
    if verbose:
        worst = np.abs(g - want.grad) / (SC.GRAD_TOL["rtol"] * np.abs(want.grad) + SC.GRAD_TOL["atol"] * want.scale)
        print(f"    gradient: worst error / bound off the undecided elements {np.max(np.where(want.undecided, 0.0, worst)):.3e}; "
              f"undecided {int(want.undecided_per_set.sum())}, taking the other decision {int((~within(want.grad) & want.undecided).any(axis=1).sum())}")
    assert ok.all(), (name, int((~ok).sum()))


def weights_from_gradient(name, grad):
    """The element weights a gradient implies, ``[B, E]``: the gradient over ``coef / kept * (p - target)`` on the channel where
    that is largest (multiclass) or on the element's own channel; NaN where the model's derivative is too small to divide by."""
    case = CASES[name]
    want = model(name)
    _, _, d = _elements(name)
    g = grad.cpu().numpy().astype(np.float64)
    sets = want.coef.size
    unit = want.coef / np.maximum(np.atleast_1d(want.kept), 1)
    if case.per_sample and case.reduction == "mean":
        unit = unit / sets
    unit = np.broadcast_to(unit[:, None], (sets, want.weight.size // sets)).reshape(case.B, -1)
    if case.mode == "multiclass":
        c = np.abs(d).argmax(axis=1)[:, None]
        dd, gg = np.take_along_axis(d, c, 1).reshape(case.B, -1), np.take_along_axis(g, c, 1).reshape(case.B, -1)
    else:
        dd, gg = d.reshape(case.B, -1), g.reshape(case.B, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.abs(dd) > 0.05, gg / (unit * dd), np.nan)
