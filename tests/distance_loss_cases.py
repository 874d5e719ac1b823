"""Cases and a float64 numpy model of the distance-map losses (losses/distance_losses.py): values and gradients.

THE MODEL restates the definitions, nothing of the implementation: softmax / sigmoid in float64 on the float32 logits widened, the 0 / 1
target, the signed maps from ``distance_cases.restate`` (brute force, scipy above its limit) or, with spacing, ``scipy_squared`` -- positive
outside the object, negative inside, an entry without a boundary as 0 --, the mean over the elements that are not ignored, and the
gradient by the chain rule with the maps as constants.

THE CASES are the shapes at which the kernels of csrc/ptb_distance_loss.hip can go wrong, all tiny: rows of 5, 8 and 67 (peeled and
16-byte accesses), a buffer one element off 16-byte alignment, samples on both sides of a workgroup's 1024 positions and of the
transform's 256-position chunk, channel counts on both sides of every register bucket of the softmax (4 / 8 / 16) and above them (the
second sweep), samples that lack a class or are one class everywhere (the +-inf maps), a class subset without channel 0, an ignored
region that touches an object, a volume, anisotropic spacing, all three modes, probabilities instead of logits, and logits of +-60."""
import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np

import distance_cases as DC

BOUNDARY, HAUSDORFF = "boundary", "hausdorff"
SPAN = 1024                  # positions of a sample per workgroup of the loss kernels
IGNORE = 255


class Case(NamedTuple):
    name: str
    mode: str = "multiclass"
    B: int = 2
    C: int = 3
    spatial: Tuple[int, ...] = (6, 8)
    classes: Optional[Tuple[int, ...]] = None
    ignore: bool = False
    spacing: Optional[Tuple[float, ...]] = None
    from_logits: bool = True
    offset: bool = False     # the logits start one element off 16-byte alignment
    extreme: bool = False    # logits of +-60 at a few pixels
    pattern: str = "blobs"   # blobs | missing (sample 0 lacks class 1, sample 1 is class 1 everywhere)
    seed: int = 0


def _cases():
    c = [Case("w5", spatial=(6, 5)), Case("w8", spatial=(6, 8)), Case("w67", spatial=(5, 67)),
         Case("offset", spatial=(6, 8), offset=True), Case("offset_binary", mode="binary", C=1, spatial=(6, 8), offset=True)]
    for shape in ((31, 33), (32, 32), (25, 41), (15, 17), (16, 16), (1, 257)):
        c.append(Case(f"s{shape[0] * shape[1]}", spatial=shape, B=1 if shape[0] * shape[1] > 300 else 2))
    for C in (1, 3, 4, 5, 8, 9, 16, 17):
        c.append(Case(f"c{C}", C=C, spatial=(5, 9)))
    c += [Case("missing", pattern="missing", spatial=(7, 8)), Case("missing_w5", pattern="missing", spatial=(7, 5)),
          Case("subset", C=4, classes=(1, 3)), Case("subset_order", C=5, classes=(4, 2, 1), spatial=(6, 7)),
          Case("subset_c17", C=17, classes=(16, 3), spatial=(5, 9)),
          Case("ignore", ignore=True, spatial=(9, 8)), Case("ignore_w5", ignore=True, spatial=(9, 5), C=4, classes=(1, 2, 3)),
          Case("volume", spatial=(5, 6, 7)), Case("volume_w8", spatial=(3, 5, 8), C=4),
          Case("spacing", spatial=(7, 8), spacing=(2.0, 0.5)), Case("spacing_volume", spatial=(5, 6, 7), spacing=(2.5, 0.7, 0.7)),
          Case("binary", mode="binary", C=1, spatial=(9, 8)), Case("binary_ignore", mode="binary", C=1, spatial=(9, 7), ignore=True),
          Case("multilabel", mode="multilabel", C=3, spatial=(7, 8)), Case("multilabel_subset", mode="multilabel", C=5, classes=(3, 1), spatial=(7, 5)),
          Case("multilabel_ignore", mode="multilabel", C=2, spatial=(6, 8), ignore=True),
          Case("probabilities", from_logits=False, spatial=(7, 8)), Case("probabilities_binary", mode="binary", C=1, from_logits=False, spatial=(7, 5)),
          Case("extreme", extreme=True, spatial=(8, 8)), Case("extreme_c17", extreme=True, C=17, spatial=(5, 8)),
          Case("extreme_binary", mode="binary", C=1, extreme=True, spatial=(8, 7))]
    return {k.name: k for k in c}


CASES = _cases()
CHUNKED = "subset_chunks"    # K = 4 maps per sample for the chunked run
CASES[CHUNKED] = Case(CHUNKED, C=5, classes=(1, 2, 3, 4), spatial=(6, 7))
ALPHA_CASES = ("w5", "w8", "c17", "missing", "spacing", "volume", "binary", "multilabel", "probabilities")        # alpha = 1 as well
EXTREME_LOGIT = 60.0


# ---------------------------------------------------------------------------------------------------------------- inputs
def _blobs(rng, shape, n):
    """labels in [0, n): a coarse random map blown up, so that every class has objects with a boundary"""
    coarse = rng.integers(0, n, tuple((s + 2) // 3 for s in shape))
    a = coarse
    for axis in range(len(shape)):
        a = np.repeat(a, 3, axis=axis)
    return a[tuple(slice(0, s) for s in shape)]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """``(x float32 [B, C, *spatial], target)`` of a case: int64 labels ``[B, *spatial]`` (multiclass) or float32 0 / 1 ``[B, C, *spatial]``; the
    logits keep every probability a safe distance from the 0.5 at which the Hausdorff form thresholds."""
    case = CASES[name]
    rng = np.random.default_rng(1000 + sum(map(ord, name)) + case.seed)
    shape = (case.B, case.C) + case.spatial
    x = rng.normal(0.0, 2.0, shape)
    if case.extreme:
        flat = x.reshape(case.B, case.C, -1)
        for i, p in enumerate(rng.choice(flat.shape[2], 4, replace=False)):
            flat[i % case.B, rng.integers(case.C), p] = EXTREME_LOGIT if i % 2 else -EXTREME_LOGIT
    if not case.from_logits:
        x = _softmax(x) if case.mode == "multiclass" else 1.0 / (1.0 + np.exp(-x))
    x = x.astype(np.float32)
    if case.mode == "multiclass":
        t = np.stack([_blobs(rng, case.spatial, case.C) for _ in range(case.B)]).astype(np.int64)
        if case.pattern == "missing":
            t[0][t[0] == 1] = 0
            t[1][...] = 1
        if case.ignore:
            t[:, ..., 2:5, 1:4] = IGNORE                       # a block inside the map: it touches whatever objects lie there
    else:
        t = np.stack([np.stack([_blobs(rng, case.spatial, 2) for _ in range(case.C)]) for _ in range(case.B)]).astype(np.float32)
        if case.pattern == "missing":
            t[0, 0], t[1, 0] = 0.0, 1.0
        if case.ignore:
            t[:, :, ..., 2:5, 1:4] = IGNORE
    p = probabilities(case, x)
    assert np.abs(p - 0.5).min() > 1e-6, name                  # the threshold is decided the same way in float32
    x.setflags(write=False)
    t.setflags(write=False)
    return x, t


def _softmax(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def probabilities(case, x):
    x = np.asarray(x, dtype=np.float64)
    if not case.from_logits:
        return x
    return _softmax(x) if case.mode == "multiclass" else 1.0 / (1.0 + np.exp(-x))


def selected(case):
    return tuple(case.classes) if case.classes is not None else tuple(range(case.C))


# ---------------------------------------------------------------------------------------------------------------- maps
def signed_maps(objects, dims, spacing=None):
    """float64 signed distances of boolean ``objects`` ``[*stack, *spatial]``: the distance to the object outside it, minus the distance to
    the outside inside it; ``inf`` / ``-inf`` throughout an entry whose object is empty / fills it"""
    objects = np.asarray(objects, dtype=bool)
    if spacing is None:
        out_sq, in_sq = DC.restate(objects, dims).reshape(objects.shape), DC.restate(~objects, dims).reshape(objects.shape)
        to_object, to_outside = DC.as_float(out_sq), DC.as_float(in_sq)
    else:
        to_object = np.sqrt(DC.scipy_squared(objects, dims, sampling=spacing).reshape(objects.shape))
        to_outside = np.sqrt(DC.scipy_squared(~objects, dims, sampling=spacing).reshape(objects.shape))
    return np.where(objects, -to_outside, to_object)


def signed_squared(objects, dims):
    """int64 sign * d^2 with +-(2^31 - 1) for the infinities: the int32 form of ``class_distance_maps(squared=True)``"""
    objects = np.asarray(objects, dtype=bool)
    out_sq, in_sq = DC.restate(objects, dims).reshape(objects.shape), DC.restate(~objects, dims).reshape(objects.shape)
    return np.where(objects, -in_sq, out_sq)


def _no_inf(a):
    return np.where(np.isfinite(a), a, 0.0)


# ---------------------------------------------------------------------------------------------------------------- the model
class Model(NamedTuple):
    loss: np.ndarray             # float64 [] or [B]
    grad: np.ndarray             # float64 [B, C, *spatial]: of loss (mean) or loss.sum() (none)
    mean_abs_term: float         # mean |term| over the counted elements
    field_max: float             # largest |phi| (boundary) / F (Hausdorff) of the case
    coef: np.ndarray             # [1] or [B]: 1 / count


@functools.lru_cache(maxsize=None)
def model(name, kind, alpha=2.0, reduction="mean"):
    case = CASES[name]
    x, t = inputs(name)
    dims = len(case.spatial)
    cls = list(selected(case))
    p_all = probabilities(case, x)
    p = p_all[:, cls]
    if case.mode == "multiclass":
        valid = np.broadcast_to((t != IGNORE)[:, None] if case.ignore else np.ones_like(t, bool)[:, None], p.shape)
        g = t[:, None] == np.asarray(cls).reshape((1, -1) + (1,) * dims)
    else:
        d = t[:, cls]
        valid = d != IGNORE if case.ignore else np.ones(d.shape, bool)
        g = d > 0.5
    phi_t = _no_inf(signed_maps(g & valid, dims, case.spacing))
    if kind == BOUNDARY:
        field = phi_t
        term = p * field
        dterm = field
    else:
        phi_p = _no_inf(signed_maps(p > 0.5, dims, case.spacing))
        field = np.abs(phi_p) ** alpha + np.abs(phi_t) ** alpha
        term = (p - g) ** 2 * field
        dterm = 2.0 * (p - g) * field
    term = np.where(valid, term, 0.0)
    dterm = np.where(valid, dterm, 0.0)
    axes = tuple(range(1, p.ndim))
    if reduction == "mean":
        count = np.asarray([valid.sum()], dtype=np.float64)
        loss = term.sum() / count[0]
    else:
        count = valid.sum(axis=axes).astype(np.float64)
        loss = term.sum(axis=axes) / count
    coef = 1.0 / count
    tk = dterm * (coef.reshape((-1,) + (1,) * (p.ndim - 1)) if reduction != "mean" else coef[0])
    tc = np.zeros(p_all.shape)
    tc[:, cls] = tk
    if not case.from_logits:
        grad = tc
    elif case.mode == "multiclass":
        grad = p_all * (tc - (p_all * tc).sum(axis=1, keepdims=True))
    else:
        grad = p_all * (1.0 - p_all) * tc
    n = max(int(valid.sum()), 1)
    return Model(np.asarray(loss), grad, float(np.abs(term).sum() / n), float(np.abs(field).max()), coef)


def extreme_pixels(case, x):
    """[B, 1, *spatial]: the pixels that hold a logit of +-60"""
    return (np.abs(np.asarray(x)) >= EXTREME_LOGIT).any(axis=1, keepdims=True) if case.extreme else np.zeros((x.shape[0], 1) + x.shape[2:], bool)


def module_arguments(case, kind, alpha=2.0, reduction="mean"):
    kw = dict(mode=case.mode, classes=list(case.classes) if case.classes is not None else None, from_logits=case.from_logits,
              ignore_index=IGNORE if case.ignore else None, spacing=case.spacing, reduction=reduction)
    if kind == HAUSDORFF:
        kw["alpha"] = alpha
    return kw
