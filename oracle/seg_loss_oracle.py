"""Oracle (test infrastructure only): float64 model of what the segmentation-loss kernels of csrc/ptb_losses.hip SUM -- not of the
final losses, which oracle/losses_oracle.py restates (``lf.py`` = pytorch_toolbelt/losses/functional.py, ``dice.py`` / ``jaccard.py`` /
``focal.py`` = pytorch_toolbelt/losses/<name>; the formulas are the ones losses_oracle.py cites).

* sigmoid focal (lf.py:61-94): sum_i L_i, sum_i F_i and the element-wise L map, hard labels one-hot over C or dense targets;
* region statistics (dice.py:68-111): I_c = sum p t, P_c = sum p, T_c = sum t with p = softmax / sigmoid / the given probabilities;
* softmax focal (lf.py:110-173): the two sums and the per-pixel map;
* the region epilogue (dice.py:112-131, jaccard.py:95-113): the scalar loss and d loss / d (sums) from the sums.

The numpy half gives values.  The torch half restates the same chains op for op the way the reference writes them, for any dtype: in
float64 autograd differentiates it against upstream coefficients (the gradient reference), in float32 it is the reference's own
evaluation (how much two correct float32 evaluations may differ: the conditioning of a test case).

Two conventions are the kernels', where the reference leaves the quantity unused: an ignored element's target counts as 0 in its
focal TERM (the reference holds ignore_index there, and reads the term sum only with normalized=True, which masks those terms), and
that term is a constant for the gradient (the backward kernels write 0 for every ignored element)."""
import numpy as np

from . import losses_oracle as LO

F64 = np.float64
PROB_SOFTMAX, PROB_SIGMOID, PROB_IDENTITY = 0, 1, 2


# ------------------------------------------------------------------------------------------------- numpy float64: values
def targets(C, labels=None, dense=None, ignore=None):
    """(t, ign), both [B, C, HW]: float64 targets (0 where ignored) and the mask of ignored elements.  Hard labels [B, HW]: one-hot
    over C, a pixel whose label equals ``ignore`` is ignored in every class (focal.py:88-105, dice.py:90-102), any other label
    outside [0, C) raises like F.one_hot.  Dense targets [B, C, HW]: the elements equal to ``ignore`` (lf.py:90-94, dice.py:104-111)."""
    if labels is not None:
        labels = np.asarray(labels)
        pix = (labels == ignore) if ignore is not None else np.zeros(labels.shape, dtype=bool)
        if not (pix | ((labels >= 0) & (labels < C))).all():
            raise RuntimeError("Class values must be smaller than num_classes.")
        t = (labels[:, None, :] == np.arange(C)[None, :, None]) & ~pix[:, None, :]
        return t.astype(F64), np.broadcast_to(pix[:, None, :], t.shape).copy()
    d = np.asarray(dense, dtype=F64)
    ign = (d == ignore) if ignore is not None else np.zeros(d.shape, dtype=bool)
    return np.where(ign, 0.0, d), ign


def sigmoid_focal(x, t, ign, gamma=2.0, alpha=None, threshold=None, class_weights=None, mask_term=False):
    """(L map, sum L, sum F) of lf.py:61-94.  1 - pt is formed as t (1 - p) + (1 - t) p from both sigmoids, without cancellation."""
    x = np.asarray(x, dtype=F64)
    p, q = LO._sigmoid(x), LO._sigmoid(-x)
    ce = LO._bce_with_logits(x, t)                                                  # :66
    pt, omp = p * t + q * (1.0 - t), q * t + p * (1.0 - t)                          # :67
    if threshold is None:
        f = np.power(omp, gamma)                                                    # :71
    else:
        f = np.where(pt < threshold, 1.0, np.power(omp / (1.0 - threshold), gamma))  # :73-76
    L = f * ce                                                                      # :78
    if alpha is not None:
        L = L * (alpha * t + (1.0 - alpha) * (1.0 - t))                             # :80-81
    if class_weights is not None:
        L = L * np.asarray(class_weights, dtype=F64)[None, :, None]                 # :83-88
    L = np.where(ign, 0.0, L)                                                       # :90-94
    F = np.where(ign, 0.0 if mask_term else f, f)
    return L, L.sum(), F.sum()


def probabilities(x, prob):
    x = np.asarray(x, dtype=F64)
    return LO._softmax(x, 1) if prob == PROB_SOFTMAX else (LO._sigmoid(x) if prob == PROB_SIGMOID else x)


def region_stats(x, t, ign, prob):
    """(I, P, T), each [C]: p * mask and t * mask summed over batch and pixels (dice.py:85-111)."""
    p = np.where(ign, 0.0, probabilities(x, prob))
    t = np.where(ign, 0.0, t)
    return (p * t).sum(axis=(0, 2)), p.sum(axis=(0, 2)), t.sum(axis=(0, 2))


def softmax_focal(x, labels, class_weights=None, gamma=2.0, threshold=None, ignore_label=-100):
    """(per-pixel map [B, HW], its sum, the sum of ALL focal terms) of lf.py:110-173: the terms are not masked (:161-164), an ignored
    pixel's target is class 0 (:139).  1 - p of the label's class is the other classes' share of the denominator, not a difference."""
    x = np.asarray(x, dtype=F64)
    labels = np.asarray(labels)
    C = x.shape[1]
    ign = labels == ignore_label                                                    # :137
    tgt = np.where(ign, 0, labels)
    if tgt.size and (tgt.min() < 0 or tgt.max() >= C):
        raise RuntimeError("Class values must be smaller than num_classes.")
    oh = (tgt[:, None, :] == np.arange(C)[None, :, None]).astype(F64)               # :139-140
    e = np.exp(x - x.max(axis=1, keepdims=True))
    d = e.sum(axis=1, keepdims=True)
    p, others = e / d, (e * (1.0 - oh)).sum(axis=1, keepdims=True) / d              # :141
    pt = (1.0 - oh) * p + oh * others                                               # :142
    bce = LO._bce_with_logits(x, oh)                                                # :144
    f = np.power(pt, gamma) if threshold is None else np.where(pt < threshold, 1.0, np.power(pt / threshold, gamma))   # :148-151
    loss = f * bce
    if class_weights is not None:
        loss = loss * np.asarray(class_weights, dtype=F64)[None, :, None]
    pix = loss.sum(axis=1) * ~ign                                                   # :159
    return pix, pix.sum(), f.sum()


def region_epilogue(focal_sum, I, P, T, focal_scale=0.0, dice_weight=1.0, jaccard_weight=0.0, smooth=0.0, eps=1e-7, log_loss=False,
                    class_mask=None, n_selected=None):
    """(loss, coef [2 + 2C]) of ``focal_scale * sum L + dice_weight * Dice + jaccard_weight * Jaccard``: each region loss is the mean
    over the ``n_selected`` classes of ``class_mask`` of 1 - score (or -log max(score, eps)), zero for a class without positives;
    coef = d loss / d (sum L, sum F, I[C], P[C]).  The clamps pass the gradient where they do not bind (torch's clamp_min)."""
    I, P, T = (np.asarray(v, dtype=F64) for v in (I, P, T))
    C = I.shape[0]
    sel = np.ones(C, dtype=bool) if class_mask is None else np.asarray(class_mask).astype(bool)
    n = float(C if n_selected is None else n_selected)
    active = T > 0

    def tail(score):
        if log_loss:
            loss, ds = -np.log(np.maximum(score, eps)), np.where(score >= eps, -1.0 / np.maximum(score, eps), 0.0)
        else:
            loss, ds = 1.0 - score, -np.ones_like(score)
        return np.where(active & sel, loss, 0.0), np.where(active & sel, ds, 0.0)

    loss, gI, gP = focal_scale * float(focal_sum), np.zeros(C), np.zeros(C)
    if dice_weight != 0.0:
        num, card = 2.0 * I + smooth, P + T + smooth
        den = np.maximum(card, eps)
        l, ds = tail(num / den)
        loss += dice_weight * l.sum() / n
        gI += dice_weight * ds * 2.0 / den
        gP += dice_weight * ds * np.where(card >= eps, -num / den ** 2, 0.0)
    if jaccard_weight != 0.0:
        num, uni = I + smooth, P + T - I + smooth
        den = np.maximum(uni, eps)
        l, ds = tail(num / den)
        loss += jaccard_weight * l.sum() / n
        dden = np.where(uni >= eps, num / den ** 2, 0.0)
        gI += jaccard_weight * ds * (1.0 / den + dden)
        gP += jaccard_weight * ds * -dden
    return loss, np.concatenate([[focal_scale, 0.0], gI / n, gP / n])


# ------------------------------------------------------------------------------------------------- torch, any dtype: the reference's chains
def torch_targets(C, labels=None, dense=None, ignore=None, dtype=None):
    import torch

    t, ign = targets(C, None if labels is None else np.asarray(labels), None if dense is None else np.asarray(dense), ignore)
    return torch.from_numpy(t).to(dtype), torch.from_numpy(ign)


def torch_sigmoid_focal(x, t, ign, gamma=2.0, alpha=None, threshold=None, class_weights=None, mask_term=False):
    """(L map, F map) the way lf.py:61-94 writes them; an ignored element's term is a constant (see the module docstring)."""
    import torch

    p = torch.sigmoid(x)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")
    pt = p * t + (1 - p) * (1 - t)
    if threshold is None:
        f = (1.0 - pt).pow(gamma)
    else:
        f = ((1.0 - pt) / (1 - threshold)).pow(gamma)
        f = torch.where(pt < threshold, torch.ones_like(f), f)
    L = f * ce
    if alpha is not None:
        L = L * (alpha * t + (1 - alpha) * (1 - t))
    if class_weights is not None:
        L = L * class_weights.to(x.dtype).view(1, -1, 1)
    L = torch.where(ign, torch.zeros_like(L), L)
    F = torch.where(ign, torch.zeros_like(f) if mask_term else f.detach(), f)
    return L, F


def torch_region_stats(x, t, ign, prob):
    """[3, C] the way dice.py:68-111 forms it: activation, p * mask, t * mask, sums over (0, 2)."""
    import torch

    p = x.log_softmax(dim=1).exp() if prob == PROB_SOFTMAX else (torch.nn.functional.logsigmoid(x).exp() if prob == PROB_SIGMOID else x)
    keep = (~ign).to(x.dtype)
    p, t = p * keep, t * keep
    return torch.stack([(p * t).sum(dim=(0, 2)), p.sum(dim=(0, 2)), t.sum(dim=(0, 2))])


def torch_softmax_focal(x, labels, class_weights=None, gamma=2.0, threshold=None, ignore_label=-100):
    """(per-pixel map, F map) the way lf.py:137-159 writes them."""
    import torch

    ign = labels == ignore_label
    oh = torch.nn.functional.one_hot(labels.masked_fill(ign, 0), x.shape[1]).permute(0, 2, 1).to(x.dtype)
    probs = torch.softmax(x, dim=1)
    pt = (1 - oh) * probs + oh * (1 - probs)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(x, oh, reduction="none")
    if threshold is None:
        f = pt.pow(gamma)
    else:
        f = (pt / threshold).pow(gamma)
        f = torch.where(pt < threshold, torch.ones_like(f), f)
    loss = f * loss
    if class_weights is not None:
        loss = loss * class_weights.to(x.dtype).view(1, -1, 1)
    return loss.sum(dim=1) * (~ign).to(x.dtype), f


def torch_region_epilogue(focal_sum, stats, focal_scale=0.0, dice_weight=1.0, jaccard_weight=0.0, smooth=0.0, eps=1e-7, log_loss=False,
                          class_mask=None, n_selected=None):
    """The scalar loss from the sums, dice.py:112-131 / jaccard.py:95-113 (and lf.py:221-247, :188-218 for the scores)."""
    import torch

    I, P, T = stats[0], stats[1], stats[2]
    C = I.shape[0]
    sel = torch.ones(C, dtype=torch.bool) if class_mask is None else torch.as_tensor(np.asarray(class_mask).astype(bool))
    n = float(C if n_selected is None else n_selected)

    def finish(scores):
        loss = -torch.log(scores.clamp_min(eps)) if log_loss else 1.0 - scores
        return (loss * (T > 0).to(loss.dtype))[sel].sum() / n

    loss = focal_scale * focal_sum if focal_scale != 0.0 else torch.zeros((), dtype=I.dtype)
    if dice_weight != 0.0:
        loss = loss + dice_weight * finish((2.0 * I + smooth) / (P + T + smooth).clamp_min(eps))
    if jaccard_weight != 0.0:
        loss = loss + jaccard_weight * finish((I + smooth) / (P + T - I + smooth).clamp_min(eps))
    return loss
