"""Grey and binary morphology with a flat structuring element, on the device the tensors are on: erosion, dilation, opening, closing, the
morphological gradient and the two top-hats -- the clean-up step after a segmentation model, and the boundary target of a label map::

    sem = binary_opening(fill_holes(sem), disk(2))            # drop specks and spurs thinner than 5 positions, as a bool mask
    edge = morphological_gradient(sem.to(torch.uint8), 3)     # dilation - erosion: the boundary band of every class change
    peaks = white_tophat(image, disk(15))                     # what an opening removes: bright detail smaller than the disk

The reference has no counterpart, so the names and meanings below are this library's.  CUDA tensors run the HIP kernels of
``csrc/ptb_morphology.hip`` (a missing kernel is an error, never a silent host computation, and never torch ops), CPU tensors take the numpy form
below with the same bits -- the device the caller names decides.

DEFINITIONS.  The footprint ``F`` has shape ``(fh, fw)`` and anchor ``(fh // 2, fw // 2)``; its offsets are ``O = {(i - fh // 2, j - fw // 2) : F[i, j]}``.

* ``E(x)(p) = min over o in O of x(p + o)`` (erosion); ``D(x)(p) = max over o in O of x(p - o)`` (dilation: the REFLECTED footprint, scipy's
  convention, not OpenCV's -- it matters for even and asymmetric footprints).
* ``opening = D o E``, ``closing = E o D``; ``morphological_gradient = D - E``, ``white_tophat = x - opening``, ``black_tophat = closing - x``.
* ``border_value=None``: positions outside the entry never take part; a window that lies wholly outside gives the dtype's highest value
  (``+inf`` for floats) for E and the lowest for D.  A scalar ``border_value``: outside positions hold it; it must be exact in the dtype.
  The binary functions default to 0, like scipy.
* Values are only selected, so results are exact in the input's dtype.  They are compared as the ordered 32-bit keys of their float32 value
  (``relax_order`` of the kernels): ``-0`` counts as ``+0`` and comes back as ``+0``; a NaN WITH THE SIGN BIT CLEAR LIES ABOVE ``+inf``, ONE WITH IT SET BELOW
  ``-inf``, so the usual NaN wins a dilation and loses an erosion.  (The one key 0xFFFFFFFF means "nothing took part"; the NaN that maps to it reads as that.)
* The three differences subtract in the dtype: integers saturate, floats take one float32 subtraction rounded once to the dtype.  For a
  mask, pass ``mask.to(torch.uint8)``: saturating subtraction of 0 / 1 is the set difference.
* The binary functions take a label map and the object rule of ``skeletonize`` / ``distance_transform``: ``labels != background``, or
  ``labels == foreground``; the result is ``bool``.

``footprint``: an int ``n`` (an ``n x n`` square), ``(h, w)``, or a 2-D bool / 0-1 array or tensor (read on the host); ``disk``, ``diamond`` and ``rectangle``
make the usual ones.  Every offset must satisfy ``|dy|, |dx| <= 31``, and the footprint may have at most 256 horizontal runs (maximal
stretches of set columns in a row; a disk, diamond or rectangle has one per row).  An empty footprint is a ``ValueError``.

Left out: volumes (``dims=3``; a 3-D tensor is a stack of planes), footprints beyond radius 31, non-flat (weighted) structuring elements,
gradients (autograd), hit-or-miss transforms, and the use of these kernels inside ``surface.py`` and the soft skeleton.
"""
import numpy as np
import torch

from .. import _native as N
from . import _maps as M

__all__ = ["erosion", "dilation", "opening", "closing", "morphological_gradient", "white_tophat", "black_tophat",
           "binary_erosion", "binary_dilation", "binary_opening", "binary_closing", "disk", "diamond", "rectangle"]

_EROSION, _DILATION, _OPENING, _CLOSING, _GRADIENT, _WHITE, _BLACK = range(7)      # PTB_MORPH_*
_EQUAL, _NOT_EQUAL = 0, 1                       # PTB_THIN_EQUAL / PTB_THIN_NOT_EQUAL
REACH, MAX_RUNS = 31, 256                       # PTB_MORPH_REACH, PTB_MORPH_MAX_RUNS
STRIP, BAND = 192, 128                          # csrc/ptb_morphology.hip (ptb_morphology_geometry): the columns and rows a workgroup of the grey walk owns
BIT_WORDS, BIT_BAND = 62, 64                    # ... and the 32-column words and rows one of the bit-plane walk owns
_ID = np.uint32(0xFFFFFFFF)                     # the key of "nothing took part"
_RANGE = {torch.float32: (-np.inf, np.inf), torch.float16: (-np.inf, np.inf), torch.bfloat16: (-np.inf, np.inf), torch.uint8: (0.0, 255.0),
          torch.int16: (-32768.0, 32767.0)}


# ---------------------------------------------------------------------------------------------------------------- footprints
def disk(r):
    """the bool footprint ``dy^2 + dx^2 <= r^2`` of shape ``(2 r + 1, 2 r + 1)``"""
    r = M.check_int("disk", "r", r)
    if r < 0:
        raise ValueError(f"disk: r must be >= 0, got {r}")
    d = np.arange(-r, r + 1)
    return d[:, None] ** 2 + d[None, :] ** 2 <= r * r


def diamond(r):
    """the bool footprint ``|dy| + |dx| <= r`` of shape ``(2 r + 1, 2 r + 1)``"""
    r = M.check_int("diamond", "r", r)
    if r < 0:
        raise ValueError(f"diamond: r must be >= 0, got {r}")
    d = np.abs(np.arange(-r, r + 1))
    return d[:, None] + d[None, :] <= r


def rectangle(h, w):
    """the full bool footprint of shape ``(h, w)``"""
    h, w = M.check_int("rectangle", "h", h), M.check_int("rectangle", "w", w)
    if h < 1 or w < 1:
        raise ValueError(f"rectangle: h and w must be >= 1, got {h} and {w}")
    return np.ones((h, w), bool)


def _footprint(what, fp):
    """``(offsets int [n, 2], runs int32 [m * 3])`` of a footprint argument: the (dy, dx) of its set entries, and its horizontal runs (dy, a, b)"""
    if isinstance(fp, (int, np.integer)) and not isinstance(fp, (bool, np.bool_)):
        fp = (fp, fp)
    if isinstance(fp, (tuple, list)) and len(fp) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in fp):
        if fp[0] < 1 or fp[1] < 1:
            raise ValueError(f"{what}: a footprint size must be >= 1, got {tuple(fp)}")
        F = np.ones((int(fp[0]), int(fp[1])), bool)
    else:
        try:
            F = fp.detach().cpu().numpy() if isinstance(fp, torch.Tensor) else np.asarray(fp)
        except Exception:
            raise TypeError(f"{what}: footprint must be an int, (h, w) or a 2-D bool / 0-1 array or tensor, got {type(fp).__name__}") from None
        if F.ndim != 2 or F.dtype == object or not np.isin(F, (0, 1)).all():
            raise ValueError(f"{what}: footprint must be an int, (h, w) or a 2-D array of bool / 0 / 1, got shape {F.shape} of {F.dtype}")
        F = F != 0
    ii, jj = np.nonzero(F)
    if not ii.size:
        raise ValueError(f"{what}: the footprint is empty")
    off = np.stack([ii - F.shape[0] // 2, jj - F.shape[1] // 2], axis=1)
    if np.abs(off).max() > REACH:
        raise ValueError(f"{what}: every footprint offset must satisfy |dy|, |dx| <= {REACH}, got up to {int(np.abs(off).max())} (shape {F.shape}, anchor {F.shape[0] // 2, F.shape[1] // 2})")
    starts = np.flatnonzero((np.diff(jj) != 1) | (np.diff(ii) != 0)) + 1         # np.nonzero is row-major: a run ends where the column jumps or the row changes
    first, last = np.concatenate([[0], starts]), np.concatenate([starts, [ii.size]]) - 1
    if first.size > MAX_RUNS:
        raise ValueError(f"{what}: the footprint has {first.size} horizontal runs, at most {MAX_RUNS}")
    return off, np.stack([off[first, 0], off[first, 1], off[last, 1]], axis=1).astype(np.int32).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- host form
def _keys(v, flip):
    """the ordered 32-bit keys of a float32 array (the kernels' relax_order); ``flip``: complemented"""
    b = np.where(v == 0, np.uint32(0), v.view(np.uint32))
    return np.where(b & np.uint32(0x80000000) != 0, ~b, b | np.uint32(0x80000000)) ^ np.uint32(flip)


def _unkeys(k, flip):
    k = k ^ np.uint32(flip)
    return np.where(k & np.uint32(0x80000000) != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _gather(a, off, outside, fold, identity):
    """``fold`` over the offsets g of ``a(p + g)``, ``a`` = ``[B, H, W]`` padded with ``outside``: shifted views, started from ``identity``"""
    H, W = a.shape[1:]
    ry, rx = int(np.abs(off[:, 0]).max()), int(np.abs(off[:, 1]).max())
    p = np.pad(a, ((0, 0), (ry, ry), (rx, rx)), constant_values=outside)
    acc = np.full(a.shape, identity, a.dtype)
    for dy, dx in off:
        fold(acc, p[:, ry + dy:ry + dy + H, rx + dx:rx + dx + W], out=acc)
    return acc


def _walk_host(v, off, dilate, border, lowest, highest):
    """E or D of the float32 maps ``v`` ``[B, H, W]``: minima of keys (a dilation: of complemented keys over the reflected offsets)"""
    flip = 0xFFFFFFFF if dilate else 0
    outside = _ID if border is None else _keys(np.array([border], np.float32), flip)[0]
    acc = _gather(_keys(v, flip), -off if dilate else off, outside, np.minimum, _ID)
    return np.where(acc == _ID, np.float32(lowest if dilate else highest), _unkeys(acc, flip))


def _grey_host(op, x, off, border):
    v = x.to(torch.float32).numpy()
    lo, hi = _RANGE[x.dtype]
    first = op in (_DILATION, _CLOSING, _BLACK)
    r = _walk_host(v, off, first, border, lo, hi)
    if op in (_OPENING, _CLOSING, _WHITE, _BLACK):
        r = _walk_host(r, off, not first, border, lo, hi)
    if op in (_GRADIENT, _WHITE, _BLACK):
        with np.errstate(invalid="ignore"):                     # (inf - inf)
            d = torch.from_numpy(_walk_host(v, off, True, border, lo, hi) - r if op == _GRADIENT else v - r if op == _WHITE else r - v)
        return (d if x.dtype.is_floating_point else d.clamp(lo, hi)).to(x.dtype)        # one float32 subtraction, rounded once / saturated
    return torch.from_numpy(r).to(x.dtype)


def _binary_host(op, obj, off, border):
    def walk(a, dilate):
        if dilate:
            return _gather(a, -off, bool(border) if border is not None else False, np.logical_or, False)
        return _gather(a, off, bool(border) if border is not None else True, np.logical_and, True)

    first = op in (_DILATION, _CLOSING)
    r = walk(obj, first)
    return walk(r, not first) if op >= _OPENING else r


# ---------------------------------------------------------------------------------------------------------------- public
def _border(what, bv, dtype):
    if bv is None:
        return None
    if isinstance(bv, (bool, np.bool_)) or not isinstance(bv, (int, float, np.integer, np.floating)):
        raise TypeError(f"{what}: border_value must be None or a number, got {bv!r}")
    bv = float(bv)
    if dtype.is_floating_point:
        exact = torch.tensor(bv, dtype=torch.float64).to(dtype).to(torch.float64).item() == bv
    else:
        exact = bv.is_integer() and M.fits(int(bv), dtype)
    if not exact:
        raise ValueError(f"{what}: border_value {bv!r} is not exact in {dtype}")
    return bv


def _grey(what, op, image, footprint, border_value, out):
    M.check_values(what, "image", image)
    _, B, _, H, W = M.extent(what, "image", image, 2)
    off, runs = _footprint(what, footprint)
    border = _border(what, border_value, image.dtype)
    M.check_out(what, out, image.dtype, image)
    if B * H * W == 0:
        res = out if out is not None else torch.empty_like(image)
    elif not image.is_cuda:
        res = _grey_host(op, image.contiguous().reshape(B, H, W), off, border).reshape(image.shape)
    else:
        x = image.contiguous()
        res = out if M.direct_out(out, x) else torch.empty(x.shape, dtype=x.dtype, device=x.device)
        ws, nbytes = M.workspace(N.load().ptb_morphology_plan, what, x.device, B, H, W, op, x.element_size())
        N.launch("ptb_morphology", x.device, x.data_ptr(), M.VALUE_CODES[x.dtype], B, H, W, op, N.int_array(runs.tolist()), len(runs) // 3, int(border is not None),
                 border or 0.0, res.data_ptr(), N.ptr(ws) or None, nbytes, what=what)
    return M.finish_out(out, res)


def _binary(what, op, labels, footprint, background, foreground, border_value, out):
    M.check_labels(what, "labels", labels)
    _, B, _, H, W = M.extent(what, "labels", labels, 2)
    off, runs = _footprint(what, footprint)
    background = M.check_int(what, "background", background, allow_none=True)
    foreground = M.check_int(what, "foreground", foreground, allow_none=True)
    if foreground is None and background is None:
        raise ValueError(f"{what}: background=None needs foreground= (there would be no object)")
    rule, value = (_NOT_EQUAL, background) if foreground is None else (_EQUAL, foreground)
    if border_value is not None and (isinstance(border_value, (float, np.floating)) or border_value not in (0, 1)):
        raise ValueError(f"{what}: border_value must be None, 0 or 1, got {border_value!r}")
    border = None if border_value is None else int(border_value)
    M.check_out(what, out, out.dtype if isinstance(out, torch.Tensor) and out.dtype == torch.uint8 else torch.bool, labels)
    if B * H * W == 0:
        res = out if out is not None else torch.empty(labels.shape, dtype=torch.bool, device=labels.device)
    elif not labels.is_cuda:
        a = labels.contiguous().reshape(B, H, W).numpy()
        eq = np.zeros(a.shape, bool) if not M.fits(value, labels.dtype) else a == (bool(value) if a.dtype == np.bool_ else value)
        res = torch.from_numpy(_binary_host(op, ~eq if rule == _NOT_EQUAL else eq, off, border)).reshape(labels.shape)
    else:
        x = labels.contiguous()
        res = out if M.direct_out(out, x) else torch.empty(x.shape, dtype=torch.bool, device=x.device)
        ws, nbytes = M.workspace(N.load().ptb_morphology_plan, what, x.device, B, H, W, op, 0)
        N.launch("ptb_binary_morphology", x.device, x.data_ptr(), M.ELEM_BYTES[x.dtype], B, H, W, rule, value, op, N.int_array(runs.tolist()), len(runs) // 3,
                 -1 if border is None else border, res.data_ptr(), N.ptr(ws) or None, nbytes, what=what)      # (a bool tensor's bytes are the uint8 the kernels write)
    return M.finish_out(out, res)


_GREY_DOC = """

    ``image``: ``[*stack, H, W]`` of ``float32``, ``float16``, ``bfloat16``, ``uint8`` or ``int16``; the entries of ``stack`` are independent and share the same launches
    (``dims=2`` only: volumes are left out).  ``footprint``, ``border_value`` and the definitions: the module docstring.  ``out``: a tensor of the
    input's dtype, shape and device that receives the result (and is returned); it may be the input.

    CUDA tensors: ONE native call -- one launch of the walk kernel, two for the compound forms with the intermediate in a workspace of the
    input's size, the differences in the store stage of the second; no torch op touches the data.  A workgroup owns ``STRIP`` columns and
    ``BAND`` rows of one entry (this module's constants, the library's ``ptb_morphology_geometry``).  Contiguous inputs are read where they lie; other strides are copied first.
    Nothing is read back, so the call is asynchronous.  The result is a function of the inputs alone: the same bits on every run.  Bad
    arguments raise before anything is launched; empty inputs return without a launch."""

_BINARY_DOC = """

    ``labels``: ``[*stack, H, W]`` of ``bool``, ``uint8``, ``int16``, ``int32`` or ``int64`` (``dims=2`` only).  The object is, with ``foreground=None``, the positions that do not
    hold ``background`` and, with ``foreground=c``, the positions that hold ``c``; a value the dtype cannot hold occurs nowhere.  ``border_value``: 0 (the
    default, like scipy), 1, or ``None`` (outside never takes part).  The result is ``bool``; ``out`` may be ``bool`` or ``uint8`` and may be the input.

    CUDA tensors: ONE native call; the walk runs on bit planes, 32 positions a word, packed from the labels in registers -- a plain
    erosion or dilation needs no workspace, an opening or closing one bit plane.  ``BIT_WORDS`` words and ``BIT_BAND`` rows a workgroup.  Otherwise as the grey functions."""


def erosion(image, footprint=3, border_value=None, out=None):
    """``E(image)``: the minimum over the footprint."""
    return _grey("erosion", _EROSION, image, footprint, border_value, out)


def dilation(image, footprint=3, border_value=None, out=None):
    """``D(image)``: the maximum over the reflected footprint."""
    return _grey("dilation", _DILATION, image, footprint, border_value, out)


def opening(image, footprint=3, border_value=None, out=None):
    """``D(E(image))``: removes bright detail the footprint does not fit into."""
    return _grey("opening", _OPENING, image, footprint, border_value, out)


def closing(image, footprint=3, border_value=None, out=None):
    """``E(D(image))``: removes dark detail the footprint does not fit into."""
    return _grey("closing", _CLOSING, image, footprint, border_value, out)


def morphological_gradient(image, footprint=3, border_value=None, out=None):
    """``D(image) - E(image)``, subtracted in the dtype (integers saturate)."""
    return _grey("morphological_gradient", _GRADIENT, image, footprint, border_value, out)


def white_tophat(image, footprint=3, border_value=None, out=None):
    """``image - opening(image)``, subtracted in the dtype (integers saturate)."""
    return _grey("white_tophat", _WHITE, image, footprint, border_value, out)


def black_tophat(image, footprint=3, border_value=None, out=None):
    """``closing(image) - image``, subtracted in the dtype (integers saturate)."""
    return _grey("black_tophat", _BLACK, image, footprint, border_value, out)


def binary_erosion(labels, footprint=3, background=0, foreground=None, border_value=0, out=None):
    """The erosion of the object of ``labels`` as a ``bool`` tensor."""
    return _binary("binary_erosion", _EROSION, labels, footprint, background, foreground, border_value, out)


def binary_dilation(labels, footprint=3, background=0, foreground=None, border_value=0, out=None):
    """The dilation of the object of ``labels`` as a ``bool`` tensor."""
    return _binary("binary_dilation", _DILATION, labels, footprint, background, foreground, border_value, out)


def binary_opening(labels, footprint=3, background=0, foreground=None, border_value=0, out=None):
    """The opening (erosion, then dilation) of the object of ``labels`` as a ``bool`` tensor."""
    return _binary("binary_opening", _OPENING, labels, footprint, background, foreground, border_value, out)


def binary_closing(labels, footprint=3, background=0, foreground=None, border_value=0, out=None):
    """The closing (dilation, then erosion) of the object of ``labels`` as a ``bool`` tensor."""
    return _binary("binary_closing", _CLOSING, labels, footprint, background, foreground, border_value, out)


for _f in (erosion, dilation, opening, closing, morphological_gradient, white_tophat, black_tophat):
    _f.__doc__ += _GREY_DOC
for _f in (binary_erosion, binary_dilation, binary_opening, binary_closing):
    _f.__doc__ += _BINARY_DOC
