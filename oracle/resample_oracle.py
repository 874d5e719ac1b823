"""Oracle (test infrastructure only): every resize of csrc/ptb_resample.hip as a float64 linear operator, and the multiscale merges
built on it.

All five F.interpolate modes of a [B, C, H, W] tensor are separable: out = Ry . X . Rx^T with one [n_out, n_in] matrix per axis.
``axis_matrix`` computes the source coordinates and indices in ``tap_dtype`` -- float32: the kernels' own arithmetic, so the operator
selects the same pixels and lerp weights; float64: the coordinates F.interpolate uses on float64 tensors -- and everything after
that in float64: the weights are widened and accumulated per (output, source) pair, the products are float64 matmuls.  The adjoint
of a resize is Ry^T . G . Rx.  The merges are written on torch float64 CPU tensors, so autograd of the same expression is their
gradient reference.

The tap rules themselves are those of oracle/tta_oracle.py (``_axis_taps``, ``_cubic_taps``, the nearest and area index rules), not
restated here."""
import numpy as np
import torch

from . import tta_oracle as AO

MODES = ("bilinear", "bicubic", "nearest", "nearest-exact", "area")
REDUCTIONS = ("sum", "mean", "gmean", "hmean", "harmonic1p", "logodd", "log1p")
LINEAR_REDUCTIONS = ("sum", "mean")
EPS = 1e-6          # the clamps of ms_pre / ms_post (kMsEps) and of the reference's harmonic_mean / logodd_mean


def nearest_index(n_in, n_out, exact, dtype=np.float32):
    """Source index of every output position for mode 'nearest' (exact=False) / 'nearest-exact' (exact=True): the rules of
    AO.nearest_resize / AO.nearest_exact_resize with the scale and the product evaluated in ``dtype``."""
    dtype = np.dtype(dtype).type
    scale = dtype(n_in / n_out)
    dst = np.arange(n_out, dtype=dtype)
    if exact:
        dst = dst + dtype(0.5)
    return np.minimum(np.floor(dst * scale).astype(np.int64), n_in - 1)


def nearest_exact_index_rational(n_in, n_out):
    """'nearest-exact' in exact rational arithmetic: min(floor((2 d + 1) n_in / (2 n_out)), n_in - 1)."""
    d = np.arange(n_out, dtype=np.int64)
    return np.minimum(((2 * d + 1) * n_in) // (2 * n_out), n_in - 1)


def area_window(n_in, n_out):
    """[start, end) of every output position's averaging window (adaptive_avg_pool start_index / end_index, integers)."""
    o = np.arange(n_out, dtype=np.int64)
    return (o * n_in) // n_out, -((-(o + 1) * n_in) // n_out)


def axis_matrix(mode, n_in, n_out, align_corners=None, tap_dtype=np.float32):
    """float64 [n_out, n_in] operator of one axis of F.interpolate(mode, align_corners)."""
    if mode not in MODES:
        raise KeyError(mode)
    dtype = np.dtype(tap_dtype).type
    M = np.zeros((n_out, n_in), dtype=np.float64)
    o = np.arange(n_out)
    if mode == "bilinear":
        i0, i1, lam = AO._axis_taps(n_in, n_out, bool(align_corners), dtype)
        np.add.at(M, (o, i0), (dtype(1) - lam).astype(np.float64))       # (1 - lambda in tap_dtype: the kernels' l0)
        np.add.at(M, (o, i1), lam.astype(np.float64))
    elif mode == "bicubic":
        idx, w = AO._cubic_taps(n_in, n_out, bool(align_corners), dtype)
        for k in range(4):                                               # clamped taps coincide at the borders: accumulate
            np.add.at(M, (o, idx[k]), w[k].astype(np.float64))
    elif mode == "area":
        lo, hi = area_window(n_in, n_out)
        for q in range(n_out):
            M[q, lo[q]:hi[q]] = 1.0 / float(hi[q] - lo[q])
    else:
        M[o, nearest_index(n_in, n_out, mode == "nearest-exact", dtype)] = 1.0
    return M


def _matrices(mode, in_hw, out_hw, align_corners, tap_dtype):
    return (axis_matrix(mode, in_hw[0], out_hw[0], align_corners, tap_dtype), axis_matrix(mode, in_hw[1], out_hw[1], align_corners, tap_dtype))


def resize(x, size, mode, align_corners=None, tap_dtype=np.float32):
    """Forward Ry . X . Rx^T of a [..., H, W] numpy array, float64."""
    Ry, Rx = _matrices(mode, x.shape[-2:], size, align_corners, tap_dtype)
    return Ry @ np.asarray(x, dtype=np.float64) @ Rx.T


def resize_adjoint(g, in_hw, mode, align_corners=None, tap_dtype=np.float32):
    """Adjoint Ry^T . G . Rx: the gradient w.r.t. a [..., H, W] input of sum(resize(x) * g), float64."""
    Ry, Rx = _matrices(mode, in_hw, g.shape[-2:], align_corners, tap_dtype)
    return Ry.T @ np.asarray(g, dtype=np.float64) @ Rx


def area_resize_f32(x, size):
    """AO.area_resize (float32 sums, window rows outer, columns inner, one division by the count) evaluated for all output pixels at
    once: pass (dy, dx) adds the window's element (dy, dx) where the window has one and 0 elsewhere, which leaves a float32 sum
    unchanged -- bit-identical to the loop over output pixels, at sizes where that loop takes minutes."""
    x = np.asarray(x, dtype=np.float32)
    (y0, y1), (x0, x1) = area_window(x.shape[-2], size[0]), area_window(x.shape[-1], size[1])
    acc = np.zeros(x.shape[:-2] + (size[0], size[1]), dtype=np.float32)
    for dy in range(int((y1 - y0).max())):
        yy, oky = np.minimum(y0 + dy, x.shape[-2] - 1), (y0 + dy < y1)
        for dx in range(int((x1 - x0).max())):
            xx, okx = np.minimum(x0 + dx, x.shape[-1] - 1), (x0 + dx < x1)
            acc = acc + np.where(oky[:, None] & okx[None, :], x[..., yy[:, None], xx[None, :]], np.float32(0))
    return acc / ((y1 - y0)[:, None] * (x1 - x0)[None, :]).astype(np.float32)


# ------------------------------------------------------------------------------------------------- merges (torch float64, autograd)
def reduce_t(stack, reduction):
    """The seven reductions over dim 0 of a float64 tensor, written out (formulas and 1e-6 clamps of ms_pre / ms_post)."""
    if reduction == "sum":
        return stack.sum(0)
    if reduction == "mean":
        return stack.mean(0)
    if reduction == "gmean":
        return torch.exp(torch.log(stack).mean(0))
    if reduction == "hmean":
        return 1.0 / torch.clamp_min((1.0 / torch.clamp_min(stack, EPS)).mean(0), EPS)
    if reduction == "harmonic1p":
        return 1.0 / (1.0 / (stack + 1.0)).mean(0) - 1.0
    if reduction == "logodd":
        p = torch.clamp(stack, EPS, 1.0 - EPS)
        e = torch.exp(torch.log(p / (1.0 - p)).mean(0))
        return e / (1.0 + e)
    if reduction == "log1p":
        return torch.exp(torch.log1p(stack).mean(0)) - 1.0
    raise KeyError(reduction)


def resize_t(x, size, mode="bilinear", align_corners=None, tap_dtype=np.float32):
    """``resize`` on a float64 torch tensor (differentiable)."""
    Ry, Rx = _matrices(mode, tuple(x.shape[-2:]), size, align_corners, tap_dtype)
    return torch.from_numpy(Ry) @ x @ torch.from_numpy(Rx.T.copy())


def unflip_t(y, code):
    """View code of the kernels: bit 1 = rows flipped, bit 2 = columns flipped (both flips are their own inverse)."""
    dims = [d for d, bit in ((-2, 2), (-1, 4)) if code & bit]
    return torch.flip(y, dims) if dims else y


def ms_merge_t(maps, size, reduction="mean", align_corners=True, views=(0,), inner="mean", mode="bilinear", tap_dtype=np.float32):
    """post(mean_s pre(resize_s(inner_v(unflip_v(y_s))))): maps[s] = float64 [V * B, C, h_s, w_s] tensor (chunk-major views); maps that
    already have the output size are not resized (the reference skips F.interpolate at offset 0)."""
    V = len(views)
    back = []
    for y in maps:
        if V > 1:
            y = reduce_t(torch.stack([unflip_t(c, v) for c, v in zip(torch.chunk(y, V, dim=0), views)]), inner)
        if tuple(y.shape[-2:]) != tuple(size):
            y = resize_t(y, size, mode, align_corners, tap_dtype)
        back.append(y)
    return reduce_t(torch.stack(back), reduction)
