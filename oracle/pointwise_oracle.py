"""Oracle (test infrastructure only) for the reference's remaining elementwise + reduce losses.

float64 numpy restatements; citations are paths under ``pytorch_toolbelt/losses/``.  The first half returns the reduced losses; the
second half is the per-element model of the kernels of csrc/ptb_pointwise.hip (value, contribution to every sum, analytic gradient)
that tests/pointwise_cases.py sweeps, with the bi-tempered losses evaluated by the reference's algorithm rather than its limit."""
import math

import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _log1pexp_neg_abs(x):
    return np.log1p(np.exp(-np.abs(x)))


def _logsigmoid(x):
    return -(np.maximum(-x, 0.0) + _log1pexp_neg_abs(x))


def _reduce(loss, reduction):
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    return loss


def soft_bce(x, t, weight=None, pos_weight=None, ignore_index=-100, reduction="mean", smooth_factor=None):
    """SoftBCEWithLogitsLoss.forward, soft_bce.py:29-46.  BCE-with-logits (torch formula):
    ``(1 - s) * x + (1 + (pw - 1) * s) * (log1p(exp(-|x|)) + max(-x, 0))``, times ``weight``; ignored elements -> 0."""
    x, t = _f64(x), _f64(t)
    s = (1 - t) * smooth_factor + t * (1 - smooth_factor) if smooth_factor is not None else t      # :30-33
    pw = _f64(pos_weight) if pos_weight is not None else 1.0
    loss = (1 - s) * x + (1 + (pw - 1) * s) * (_log1pexp_neg_abs(x) + np.maximum(-x, 0.0))         # :35-37
    if weight is not None:
        loss = loss * _f64(weight)
    if ignore_index is not None:
        loss = loss * (t != ignore_index)                                                          # :39-41
    return _reduce(loss, reduction)


def balanced_bce(x, t, gamma=1.0, ignore_index=None, reduction="mean"):
    """balanced_binary_cross_entropy_with_logits, balanced_bce.py:27-49 (the power is applied twice, :31 and :33-34)."""
    x, t = _f64(x), _f64(t)
    n_pos, n_neg = float((t == 1).sum()), float((t == 0).sum())                                    # :27-28
    pos_weight = np.float32(np.float32(n_neg) / np.float32(n_pos + n_neg + 1e-7)) ** np.float32(gamma)   # :30-31 in float32
    neg_weight = np.float32(1.0) - pos_weight                                                      # :32
    pos_term = float(np.float32(pos_weight) ** np.float32(gamma)) * t * _logsigmoid(x)             # :33
    neg_term = float(np.float32(neg_weight) ** np.float32(gamma)) * (1 - t) * _logsigmoid(-x)      # :34
    loss = -(pos_term + neg_term)                                                                  # :36
    if ignore_index is not None:
        loss = np.where(t == ignore_index, 0.0, loss)                                              # :38-39
    return _reduce(loss, reduction)


def quality_focal(x, t, beta=2.0, reduction="mean"):
    """QualityFocalLoss.forward, quality_focal_loss.py:30-45."""
    x, t = _f64(x), _f64(t)
    bce = np.maximum(x, 0.0) - x * t + _log1pexp_neg_abs(x)                                        # :33
    p = 1.0 / (1.0 + np.exp(-x))
    focal = np.abs(p - t) ** beta                                                                  # :34
    loss = focal * bce                                                                             # :35
    if reduction == "normalized":
        return loss.sum() / focal.sum()                                                            # :41-42
    return _reduce(loss, reduction)


def wing(output, target, width=5, curvature=0.5, reduction="mean"):
    """wing_loss, functional.py:250-277."""
    d = np.abs(_f64(target) - _f64(output))                                                        # :260
    c = width - width * math.log(1 + width / curvature)                                            # :268
    loss = np.where(d < width, width * np.log(1 + d / curvature), d - c)                           # :266-269
    return _reduce(loss, reduction)


def log_cosh(y_pred, y_true):
    """log_cosh_loss, functional.py:326-342: mean(z + softplus(-2 z) - log 2)."""
    z = _f64(y_pred) - _f64(y_true)
    y = -2.0 * z
    return (z + np.maximum(y, 0.0) + _log1pexp_neg_abs(y) - math.log(2.0)).mean()


def soft_ce(x, labels, smooth_factor=0.0, ignore_index=-100, reduction="mean", dim=1):
    """SoftCrossEntropyLoss.forward = label_smoothed_nll_loss(log_softmax(x, dim), ...), soft_ce.py:24-33 and
    functional.py:280-323 (the gathered dim is kept in the ignore branch, squeezed otherwise)."""
    x = _f64(x)
    z = x - x.max(axis=dim, keepdims=True)
    lprobs = z - np.log(np.exp(z).sum(axis=dim, keepdims=True))                                    # soft_ce.py:25
    tgt = np.expand_dims(np.asarray(labels, dtype=np.int64), dim)                                  # functional.py:292-293
    if ignore_index is not None:
        pad = tgt == ignore_index                                                                  # :296
        nll = -np.take_along_axis(lprobs, np.where(pad, 0, tgt), axis=dim)                         # :297-298
        smooth = -lprobs.sum(axis=dim, keepdims=True)                                              # :299
        nll, smooth = np.where(pad, 0.0, nll), np.where(pad, 0.0, smooth)                          # :303-304
    else:
        nll = -np.take_along_axis(lprobs, tgt, axis=dim).squeeze(dim)                              # :306, :309
        smooth = -lprobs.sum(axis=dim, keepdims=True).squeeze(dim)                                 # :307, :310
    if reduction == "sum":
        nll, smooth = nll.sum(), smooth.sum()
    if reduction == "mean":
        nll, smooth = nll.mean(), smooth.mean()
    return (1.0 - smooth_factor) * nll + (smooth_factor / x.shape[dim]) * smooth                   # :319-321


# ------------------------------------------------------------------------------------------------- per-element models of the kernels
# float64 numpy for what csrc/ptb_pointwise.hip computes per element / pixel / row: the value, every sum the kernel adds into its slots
# (as per-element contributions, so that a test can add them up slot by slot), and the analytic input gradient for given upstream
# coefficients.  One convention for the gradient: ``g`` is the upstream gradient on the sums and ``g_elem`` the one on the optional map,
# so that grad_i = (g[0] + g_elem_i) * dL_i/dx + g[1] * dF_i/dx  (what losses/_kernels.py fold_map_grad hands the kernels).
PW_SOFT_BCE, PW_BALANCED_BCE, PW_QFL, PW_WING, PW_LOGCOSH, PW_SOFT_F1 = range(6)
PWF_IGNORE, PWF_SMOOTH = 1, 2
PW_NSUMS = (1, 4, 2, 1, 1, 4)


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def channel_of(n, C, HW):
    """Channel index of every element of a flat [B, C, HW] tensor."""
    return (np.arange(n) // HW) % C


def pointwise(kind, x, t, flags=0, p0=0.0, p1=0.0, p2=0.0, ignore_value=0.0, chan_w=None, chan_pw=None, C=1, HW=1, g=(1.0, 0.0), g_elem=None):
    """dict(parts [4, n], sums [4], elem [n], grad [n]) of ``pw_forward<KIND>`` / ``pw_backward<KIND, false>`` on flat x, t: ``parts`` the
    per-element contribution to each of the sums ``pw_forward`` names (rows beyond PW_NSUMS[kind] are zero), ``elem`` the per-element loss
    (0 for the kinds that have none)."""
    x, t = _f64(x).reshape(-1), _f64(t).reshape(-1)
    n = x.size
    g0 = g[0] + (0.0 if g_elem is None else _f64(g_elem).reshape(-1))
    g1 = g[1]
    ig = (t == ignore_value) if flags & PWF_IGNORE else np.zeros(n, dtype=bool)
    parts = np.zeros((4, n))
    p = _sigmoid(x)
    with np.errstate(all="ignore"):
        if kind == PW_SOFT_BCE:                                                        # soft_bce.py:29-41
            c = channel_of(n, C, HW)
            w = _f64(chan_w)[c] if chan_w is not None else 1.0
            pw = _f64(chan_pw)[c] if chan_pw is not None else 1.0
            st = (1 - t) * p0 + t * (1 - p0) if flags & PWF_SMOOTH else t
            lw = 1 + (pw - 1) * st
            elem = np.where(ig, 0.0, w * ((1 - st) * x + lw * (_log1pexp_neg_abs(x) + np.maximum(-x, 0.0))))
            parts[0] = elem
            grad = np.where(ig, 0.0, g0 * w * ((1 - st) - lw * (1 - p)))
        elif kind == PW_BALANCED_BCE:                                                  # balanced_bce.py:27-40
            parts[0] = np.where(ig, 0.0, t * _logsigmoid(x))
            parts[1] = np.where(ig, 0.0, (1 - t) * _logsigmoid(-x))
            parts[2], parts[3] = t == 1.0, t == 0.0
            elem = np.zeros(n)
            grad = np.where(ig, 0.0, g[0] * t * (1 - p) - g[1] * (1 - t) * p) + 0.0 * g0
        elif kind == PW_QFL:                                                           # quality_focal_loss.py:33-35
            bce = np.maximum(x, 0.0) - x * t + _log1pexp_neg_abs(x)
            diff = p - t
            d = np.abs(diff)
            f = np.ones(n) if p0 == 0.0 else d ** p0
            # torch: pow(., 0) has gradient 0; otherwise beta d^(beta - 1) sign(p - t) p (1 - p), NaN at d == 0 for beta < 1 (inf * 0)
            df = np.zeros(n) if p0 == 0.0 else p0 * d ** (p0 - 1.0) * np.sign(diff) * p * (1 - p)
            elem = f * bce
            parts[0], parts[1] = elem, f
            grad = g0 * (df * bce + f * diff) + g1 * df
        elif kind == PW_WING:                                                          # functional.py:260-269
            diff = t - x
            d = np.abs(diff)
            elem = np.where(d < p0, p0 * np.log(1 + d / p1), d - p2)
            parts[0] = elem
            grad = -g0 * np.sign(diff) * np.where(d < p0, p0 / (p1 + d), 1.0)
        elif kind == PW_LOGCOSH:                                                       # functional.py:338-341
            z = x - t
            y = -2.0 * z
            elem = z + np.maximum(y, 0.0) + _log1pexp_neg_abs(y) - math.log(2.0)
            parts[0] = elem
            grad = g0 * np.tanh(z)
        elif kind == PW_SOFT_F1:                                                       # soft_f1.py:22-24, 63-78
            given = bool(flags & PWF_SMOOTH)
            pc = x if given else np.clip(p, p0, 1 - p0)
            pc, tt = np.where(ig, 0.0, pc), np.where(ig, 0.0, t)
            parts[0], parts[1], parts[2], parts[3] = pc * tt, pc, tt, ~ig
            elem = np.zeros(n)
            slope = np.ones(n) if given else np.where((p > p0) & (p < 1 - p0), p * (1 - p), 0.0)
            grad = np.where(ig, 0.0, (g[0] * t + g[1]) * slope) + 0.0 * g0
        else:
            raise KeyError(kind)
    return dict(parts=parts, sums=parts.sum(axis=1), elem=elem, grad=grad)


def balanced_elementwise(x, t, w, flags=0, ignore_value=0.0, g_elem=None):
    """dict(elem, grad): the ``emit_loss`` form of balanced BCE, -(w[0] t logsigmoid(x) + w[1] (1 - t) logsigmoid(-x)), 0 where ignored."""
    x, t = _f64(x).reshape(-1), _f64(t).reshape(-1)
    ig = (t == ignore_value) if flags & PWF_IGNORE else np.zeros(x.size, dtype=bool)
    p = _sigmoid(x)
    elem = np.where(ig, 0.0, -(w[0] * t * _logsigmoid(x) + w[1] * (1 - t) * _logsigmoid(-x)))
    ge = np.ones(x.size) if g_elem is None else _f64(g_elem).reshape(-1)
    return dict(elem=elem, grad=np.where(ig, 0.0, -ge * (w[0] * t * (1 - p) - w[1] * (1 - t) * p)))


def soft_ce_pixels(x, labels, eps=0.0, has_ignore=False, ignore_label=0, g_total=1.0, g_pix=None):
    """dict(nll, smooth [B, HW], sums [2], pix [B, HW], total, grad [B, C, HW], bad [B, HW]) of soft_ce_kernel / soft_ce_generic_kernel on
    [B, C, HW] logits and [B, HW] labels: a pixel that is ignored -- or whose label lies outside [0, C) (``bad``: the kernel raises its
    flag) -- contributes nothing."""
    x, labels = _f64(x), np.asarray(labels, dtype=np.int64)
    B, C, HW = x.shape
    ig = (labels == ignore_label) if has_ignore else np.zeros(labels.shape, dtype=bool)
    bad = ~ig & ((labels < 0) | (labels >= C))
    ig = ig | bad
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    z = e.sum(axis=1, keepdims=True)
    lse = (m + np.log(z))[:, 0]
    p = e / z
    safe = np.where(ig, 0, labels)
    onehot = (np.arange(C)[None, :, None] == safe[:, None, :]).astype(np.float64)
    nll = np.where(ig, 0.0, lse - np.take_along_axis(x, safe[:, None, :], axis=1)[:, 0])
    smooth = np.where(ig, 0.0, C * lse - x.sum(axis=1))
    pix = (1 - eps) * nll + eps / C * smooth
    gk = np.where(ig, 0.0, g_total + (0.0 if g_pix is None else _f64(g_pix)))[:, None, :]
    grad = gk * ((1 - eps) * (p - onehot) + eps / C * (C * p - 1.0))
    sums = np.array([nll.sum(), smooth.sum()])
    return dict(nll=nll, smooth=smooth, sums=sums, pix=pix, total=(1 - eps) * sums[0] + eps / C * sums[1], grad=grad, bad=bad)


def _log_t(u, t):
    return np.log(u) if t == 1.0 else (u ** (1.0 - t) - 1.0) / (1.0 - t)


def _exp_t(u, t):
    return np.exp(u) if t == 1.0 else np.maximum(1.0 + (1.0 - t) * u, 0.0) ** (1.0 / (1.0 - t))


def bitempered_rows(act, y, t1, t2, smoothing=0.0, iters=5, g_loss=None):
    """dict(loss [R], grad [R, K], knife [R], p [R, K], norm [R, 1]) of bi_tempered_logistic_loss (bitempered_loss.py:135-180) the way the kernels
    evaluate it -- the algorithm, not its limit: ``iters`` steps of the fixed point for t2 > 1 (:25-45) or of the bisection for t2 < 1
    (:48-75), in that order, log-sum-exp for t2 == 1; the backward is the closed form through the escort distribution (:94-104), and a
    class outside the finite support (p == 0) passes no gradient.  ``knife``: the smallest |mass - 1| over the bisection steps (inf for
    the other temperatures, and an exact mass == 1 counts as inf: a tie is decided identically in every precision) -- below it another
    precision may take the other branch.  ``norm``: the normalisation of the activations shifted by their row maximum."""
    a, y = _f64(act), _f64(y)
    R, K = a.shape
    n = a - a.max(axis=1, keepdims=True)
    knife = np.full(R, np.inf)
    with np.errstate(all="ignore"):
        if t2 == 1.0:
            norm = np.log(np.exp(n).sum(axis=1, keepdims=True))
            p = np.exp(n - norm)
        elif t2 > 1.0:
            sc = 1.0
            for it in range(iters + 1):
                z = _exp_t(n * sc, t2).sum(axis=1, keepdims=True)
                if it < iters:
                    sc = z ** (1.0 - t2)
            norm = -_log_t(1.0 / z, t2)
            p = _exp_t(n - norm, t2)
        else:
            dim = (n > -1.0 / (1.0 - t2)).sum(axis=1, keepdims=True).astype(np.float64)
            lo, hi = np.zeros((R, 1)), -_log_t(1.0 / dim, t2)
            for _ in range(iters):
                mid = (hi + lo) * 0.5
                mass = _exp_t(n - mid, t2).sum(axis=1, keepdims=True)
                knife = np.minimum(knife, np.where(mass == 1.0, np.inf, np.abs(mass - 1.0))[:, 0])
                up = mass < 1.0
                hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
            norm = (hi + lo) * 0.5
            p = _exp_t(n - norm, t2)
        ys = (1.0 - smoothing * K / (K - 1)) * y + smoothing / (K - 1) if smoothing > 0.0 else y
        e = 2.0 - t1
        loss = (ys * _log_t(ys + 1e-10, t1) - ys * _log_t(p, t1) - ys ** e / e + p ** e / e).sum(axis=1)
        q = np.where(p > 0.0, p ** t2, 0.0)
        gk = -ys * p ** (-t1) + p ** (1.0 - t1)
        w = np.where(p > 0.0, gk * q, 0.0)
        r = w.sum(axis=1, keepdims=True) / q.sum(axis=1, keepdims=True)
        gl = np.ones(R) if g_loss is None else np.broadcast_to(_f64(g_loss), (R,))
        grad = gl[:, None] * (w - r * q)
    return dict(loss=loss, grad=grad, knife=knife, p=p, norm=norm)


def bitempered_binary(x, t, t1, t2, smoothing=0.0, iters=5, has_ignore=False, ignore_value=0.0, g_sum=1.0, g_elem=None):
    """dict(elem [n], sum, grad [n], knife [n]) of BinaryBiTemperedLogisticLoss (bitempered_loss.py:223-284): rows (-x, x) against
    (1 - t, t); ignored elements contribute nothing (and are no knife edges)."""
    x, t = _f64(x).reshape(-1), _f64(t).reshape(-1)
    ig = (t == ignore_value) if has_ignore else np.zeros(x.size, dtype=bool)
    gl = g_sum + (0.0 if g_elem is None else _f64(g_elem).reshape(-1))
    r = bitempered_rows(np.stack([-x, x], axis=1), np.stack([1.0 - t, t], axis=1), t1, t2, smoothing, iters, gl)
    elem = np.where(ig, 0.0, r["loss"])
    return dict(elem=elem, sum=elem.sum(), grad=np.where(ig, 0.0, r["grad"][:, 1] - r["grad"][:, 0]), knife=np.where(ig, np.inf, r["knife"]))


def soft_f1_from_counts(tp_sum, p_sum, t_sum, eps=1e-6):
    """1 - F1 from the soft counts sum p t, sum p, sum t (soft_f1.py:22-27: TP = s0, FP = s1 - s0, FN = s2 - s0)."""
    return 1.0 - 2.0 * tp_sum / (p_sum + t_sum + eps)


def soft_f1_softmax(x, labels, eps=1e-6):
    """(loss, d loss / dx) of SoftF1Loss (soft_f1.py:30-60) on [N, C] logits and integer labels: softmax, clamp to [eps, 1 - eps], soft
    counts over the samples per class, mean over classes of 1 - F1 (the clamp has zero slope outside)."""
    x = _f64(x)
    N, C = x.shape
    e = np.exp(x - x.max(axis=1, keepdims=True))
    sm = e / e.sum(axis=1, keepdims=True)
    p = np.clip(sm, eps, 1 - eps)
    y = (np.arange(C)[None, :] == np.asarray(labels).reshape(-1, 1)).astype(np.float64)
    inter, den = (p * y).sum(axis=0), p.sum(axis=0) + y.sum(axis=0) + 1e-6
    loss = (1.0 - 2.0 * inter / den).mean()
    gp = (-2.0 * y / den + 2.0 * inter / den ** 2) / C * ((sm > eps) & (sm < 1 - eps))
    return loss, sm * (gp - (gp * sm).sum(axis=1, keepdims=True))
