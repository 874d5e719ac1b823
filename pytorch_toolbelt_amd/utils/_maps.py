"""What the label-map tools of this package share on the host: the twin of ``csrc/ptb_common.h``.  ``components``, ``distance``, ``nearest``,
``watershed``, ``reconstruct``, ``skeleton``, ``surface`` and ``instances`` (and ``rle``, ``metrics``, ``losses/distance_losses.py``) take their dtype tables, their
argument checks, the handling of ``out=``, the workspace of a native call and the host form of the distance passes from here and from no
sibling.  Private: nothing here is exported from ``utils`` or part of the interface.

Every check takes ``what`` (the public function's name, the prefix of its messages) and raises the message that function documents; where
two tools word one condition differently the differing fragment is an argument (``name``, ``note``), never a second copy of the check.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _native as N

ELEM_BYTES = {torch.bool: 1, torch.uint8: 1, torch.int16: 2, torch.int32: 4, torch.int64: 8}        # the label dtypes, and what the kernels step by
VALUE_CODES = {torch.float32: N.F32, torch.float16: N.F16, torch.bfloat16: N.BF16, torch.uint8: N.U8, torch.int16: N.I16}   # heights, grey values
CONNECTIVITIES = {2: (4, 8), 3: (6, 26)}
MAX_POSITIONS = (1 << 31) - 2        # of one call: positions are indexed in int32
MAX_SQUARED = (1 << 31) - 2          # D^2 + H^2 + W^2 of one call: every squared index distance is an int32
INT_INF = (1 << 31) - 1              # the int32 form of "no site in this entry"
HOST_INF = 1 << 62                   # the same in the int64 host form
SITES_EQUAL, SITES_NOT_EQUAL = 0, 1  # PTB_EDT_SITES_*


# ---------------------------------------------------------------------------------------------------------------- values
def fits(c, dtype):
    if dtype == torch.bool:
        return c in (0, 1)
    info = torch.iinfo(dtype)
    return info.min <= c <= info.max


def check_int(what, name, v, allow_none=False):
    if v is None and allow_none:
        return None
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{what}: {name} must be an int{' or None' if allow_none else ''}, got {v!r}")
    v = int(v)
    if not -(1 << 63) <= v < (1 << 63):
        raise ValueError(f"{what}: {name} {v} does not fit int64")
    return v


def check_tensor(what, name, t, dtypes, wording, hint=""):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype not in dtypes:
        raise TypeError(f"{what}: {name} must {wording}, got {t.dtype}{hint}")


def check_labels(what, name, t):
    check_tensor(what, name, t, ELEM_BYTES, "hold integer labels (bool, uint8, int16, int32 or int64)")


def check_values(what, name, t, or_bool=False):
    check_tensor(what, name, t, tuple(VALUE_CODES) + ((torch.bool,) if or_bool else ()),
                 f"be float32, float16, bfloat16, uint8 or int16{' or bool' if or_bool else ''}", f": pass {name}.float() if every value is exact in float32")


def spacing(what, spacing, dims):
    """``None``, or the ``(z,) y, x`` spacing as three floats (1.0 for a missing z)"""
    if spacing is None:
        return None
    try:
        sp = [float(v) for v in spacing]
    except TypeError:
        raise TypeError(f"{what}: spacing must be None or {dims} floats in {'z, ' if dims == 3 else ''}y, x order, got {spacing!r}") from None
    if len(sp) != dims:
        raise ValueError(f"{what}: spacing must have {dims} entries ({'z, ' if dims == 3 else ''}y, x) for dims={dims}, got {len(sp)}")
    if not all(math.isfinite(v) and v > 0 for v in sp):
        raise ValueError(f"{what}: spacing must be positive and finite, got {sp}")
    return [1.0] * (3 - dims) + sp


# ---------------------------------------------------------------------------------------------------------------- geometry
def check_dims(what, dims):
    if dims not in (2, 3):
        raise ValueError(f"{what}: dims must be 2 or 3, got {dims!r}")


def extent(what, name, t, dims, note="", squares=False):
    """``(stack, B, D, H, W)`` of the tensor ``t`` = ``[*stack, (D,) H, W]``: ``B`` entries of ``D x H x W`` positions, within what one call takes.
    ``squares``: the squared extents are limited too (the tools that hold squared index distances in int32)."""
    check_dims(what, dims)
    if t.dim() < dims:
        raise ValueError(f"{what}: {name} must be [*stack, {'D, ' if dims == 3 else ''}H, W] for dims={dims}, got {tuple(t.shape)}")
    stack = tuple(t.shape[:-dims])
    D = t.shape[-3] if dims == 3 else 1
    H, W = t.shape[-2], t.shape[-1]
    B = math.prod(stack)
    if B * D * H * W > MAX_POSITIONS:
        raise ValueError(f"{what}: {B * D * H * W} positions in one call; at most 2^31 - 2 = {MAX_POSITIONS}{note}: split the stack")
    total = (D * D if dims == 3 else 0) + H * H + W * W
    if squares and total > MAX_SQUARED:
        raise ValueError(f"{what}: {'D^2 + ' if dims == 3 else ''}H^2 + W^2 = {total}; at most 2^31 - 2 = {MAX_SQUARED} (squared index distances are int32)")
    return stack, B, D, H, W


def check_connectivity(what, connectivity, dims, default=None, note=""):
    """``(connectivity, full)``; ``default``: which of the two (0: faces, 1: the full neighbourhood) ``None`` stands for, if it may be given"""
    check_dims(what, dims)
    pair = CONNECTIVITIES[dims]
    if connectivity is None and default is not None:
        connectivity = pair[default]
    if isinstance(connectivity, bool) or connectivity not in pair:
        raise ValueError(f"{what}: connectivity must be {pair[0]} or {pair[1]} for dims={dims}{note}, got {connectivity!r}")
    return connectivity, connectivity == pair[1]


def check_like(what, name, t, like, dtypes=None):
    """``t`` has the shape and the device of ``like``; with ``dtypes`` (a mask: bool, uint8) it is first a tensor of one of them"""
    if dtypes is not None:
        check_tensor(what, name, t, dtypes, "be " + " or ".join(str(d)[6:] for d in dtypes))
    if t.shape != like.shape or t.device != like.device:
        raise ValueError(f"{what}: {name} must have shape {tuple(like.shape)} on {like.device}, got {tuple(t.shape)} on {t.device}")


# ---------------------------------------------------------------------------------------------------------------- out=
def check_out(what, out, dtype, like):
    if out is None:
        return
    if not isinstance(out, torch.Tensor):
        raise TypeError(f"{what}: out must be a tensor, got {type(out).__name__}")
    if out.dtype != dtype or out.shape != like.shape or out.device != like.device:
        raise ValueError(f"{what}: out must be a {dtype} tensor of shape {tuple(like.shape)} on {like.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")


def direct_out(out, *inputs):
    """can the kernels write ``out`` directly?  (contiguous, aligned, and not the storage of one of ``inputs``, which they still read)"""
    return (out is not None and out.is_contiguous() and out.data_ptr() % 16 == 0
            and all(t is None or out.untyped_storage().data_ptr() != t.untyped_storage().data_ptr() for t in inputs))


def finish_out(out, res):
    """what the caller returns: ``res``, copied into ``out`` if the kernels could not write that directly"""
    if out is None or res is out:
        return res
    out.copy_(res)
    return out


# ---------------------------------------------------------------------------------------------------------------- native calls
def scratch(nbytes, device):
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def workspace(plan, what, device, *plan_args):
    """``(tensor, bytes)``: the workspace a ``ptb_*_plan`` entry with one int64 result asks for"""
    nbytes = ctypes.c_int64()
    N.check(plan(*plan_args, ctypes.byref(nbytes)), what)
    return scratch(nbytes.value, device), nbytes.value


def check_max_sweeps(what, max_sweeps, default):
    if max_sweeps is None:
        return default
    max_sweeps = check_int(what, "max_sweeps", max_sweeps)
    if not 1 <= max_sweeps < (1 << 31):
        raise ValueError(f"{what}: max_sweeps must be in [1, 2^31 - 1], got {max_sweeps}")
    return max_sweeps


def raise_not_converged(what, phases, took, max_sweeps):
    """the error of ``PTB_ENOTCONVERGED``; ``took``: the two sweep counts the call wrote, -1 for a phase that did not start"""
    phase = 0 if took[1] < 0 else 1
    raise RuntimeError(f"{what}: phase {phase + 1} (the {phases[phase]} relaxation) did not converge within max_sweeps={max_sweeps}: {took[phase]} sweeps run")


# ---------------------------------------------------------------------------------------------------------------- host form of the distance passes
def envelope_host(f, weight, inf, feat=None):
    """``g[l, i] = min_j f[l, j] + weight * (i - j)^2`` of every line ``l`` of ``f`` ([lines, n]; ``inf`` marks "no value") and, with ``feat``,
    ``feat[l, j]`` at the minimising ``j``, the SMALLEST such ``j``: ``(g, h | None)``.  Correct rather than fast: the minimum is taken shift by shift,
    ``k = |i - j|`` = 1, 2, ... on both sides at once, over the lines that hold a value at all: the left candidate ``j = i - k`` is smaller than
    every ``j`` tried before it and so wins a tie, the right one is larger and loses it.  Ends when ``weight * k^2`` exceeds every value (an
    equal one could still tie; an unreached position counts as ``inf``, so the shifts go on until every position of those lines is reached)."""
    live = (f != inf).any(axis=1)
    if not live.any():
        return f, feat
    fl = f[live]
    gl = fl.copy()
    if feat is not None:
        tl = feat[live]
        hl = tl.copy()
    for k in range(1, f.shape[1]):
        c = weight * (k * k)
        if c > gl.max():
            break
        if feat is None:
            np.minimum(gl[:, k:], fl[:, :-k] + c, out=gl[:, k:])
            np.minimum(gl[:, :-k], fl[:, k:] + c, out=gl[:, :-k])
            continue
        cand = fl[:, :-k] + c
        take = cand <= gl[:, k:]
        gl[:, k:][take] = cand[take]
        hl[:, k:][take] = tl[:, :-k][take]
        cand = fl[:, k:] + c
        take = cand < gl[:, :-k]
        gl[:, :-k][take] = cand[take]
        hl[:, :-k][take] = tl[:, k:][take]
    g = f.copy()
    g[live] = gl
    if feat is None:
        return g, None
    h = feat.copy()
    h[live] = hl
    return g, h


def edt_host(sites, sp, index=False):
    """``(squared distance, index of the nearest site within the entry | None)`` of every position of ``sites`` (bool [B, D, H, W]), one envelope
    pass per axis: int64 with ``HOST_INF`` for unit spacing, float64 with ``inf`` otherwise; int64 indices, -1 without a site"""
    B, D, H, W = sites.shape
    if sp is None:
        inf = HOST_INF
        f = np.where(sites, 0, inf).astype(np.int64)
        weights = (1, 1, 1)
    else:
        inf = np.inf
        f = np.where(sites, 0.0, inf)
        weights = tuple(s * s for s in sp)
    feat = np.where(sites, np.arange(D * H * W, dtype=np.int64).reshape(1, D, H, W), -1) if index else None
    for axis in (3, 2, 1):
        if f.shape[axis] == 1:
            continue
        lines = np.ascontiguousarray(np.moveaxis(f, axis, -1))
        flines = np.ascontiguousarray(np.moveaxis(feat, axis, -1)).reshape(-1, lines.shape[-1]) if index else None
        g, h = envelope_host(lines.reshape(-1, lines.shape[-1]), weights[axis - 1], inf, flines)
        f = np.moveaxis(g.reshape(lines.shape), -1, axis)
        if index:
            feat = np.moveaxis(h.reshape(lines.shape), -1, axis)
    return np.minimum(f, inf), np.where(f >= inf, -1, feat) if index else None
