"""Run-length codec of segmentation masks (the reference's ``pytorch_toolbelt.utils.rle``), on the host and on the device.

An encoding, with ``N = H * W`` and ``f[p] = fg[p % H][p // H]`` (column-major order, the order of ``mask.T.flatten()``): the maximal
runs of ``f`` in increasing order as ``start + 1, length`` pairs.  A run continues from the bottom of one column into the top of the
next one.

``rle_encode`` / ``rle_decode`` / ``rle_to_string`` are the reference's names and signatures; on numpy input they return what the
reference returns.  ``rle_encode_device`` / ``rle_decode_device`` take tensors: CUDA tensors run the HIP kernels of
``csrc/ptb_rle.hip`` (a missing kernel is an error, never a silent host computation), CPU tensors take torch / numpy ops with the same
results -- the device the caller names decides.
"""
import numpy as np
import torch

from .. import _native as N
from . import _maps as M

__all__ = ["rle_decode", "rle_encode", "rle_to_string", "rle_encode_device", "rle_decode_device"]

_DECODE_DTYPES = (torch.bool, torch.uint8)


# ---------------------------------------------------------------------------------------------------------------- drop-in names
def rle_encode(mask):
    """Run-length encoding of ``mask`` in column-major order: an ``int64`` array of ``start + 1, length`` pairs.

    numpy input (any rank; the order is that of ``mask.T.flatten()``) gives the reference's result: a boundary is placed wherever two
    consecutive pixels DIFFER, plus one at either end that is non-zero.  For a mask with at most one distinct non-zero value that is the
    encoding defined above.  For a mask with several non-zero values it is NOT a valid encoding -- ``[[0, 2], [1, 0]]`` gives
    ``[2, 1, 4]`` -- here as in the reference; encode such label maps per class (``rle_encode_device(mask, labels=...)``).

    A 2-D CUDA tensor returns ``rle_encode_device(mask)``, a CUDA ``int64`` tensor (foreground: ``mask != 0``).  A CUDA tensor of any
    other rank raises ``ValueError``: the reference's N-D order is not the slice-wise meaning of ``rle_encode_device``."""
    if isinstance(mask, torch.Tensor):
        if mask.is_cuda:
            if mask.dim() != 2:
                raise ValueError(f"rle_encode: a CUDA mask must be [H, W], got {tuple(mask.shape)} (rle_encode_device encodes a [B, H, W] stack slice by slice)")
            return rle_encode_device(mask)
        mask = mask.numpy()
    pixels = np.asarray(mask).T.reshape(-1)
    n = pixels.shape[0]
    edges = np.flatnonzero(pixels[1:] != pixels[:-1]).astype(np.int64) + 2       # 1-based position of the pixel behind a change
    if n and (pixels[0] or pixels[-1]):                   # the reference pads BOTH ends with a zero as soon as either end is set
        edges = np.concatenate([np.ones(1 if pixels[0] else 0, np.int64), edges, np.full(1 if pixels[-1] else 0, n + 1, np.int64)])
    pairs = edges.shape[0] // 2
    edges[1:2 * pairs:2] -= edges[0:2 * pairs:2]
    return edges


def rle_to_string(runs) -> str:
    """The runs as one space-separated string.  A tensor is copied to the host once."""
    if isinstance(runs, torch.Tensor):
        runs = runs.detach().cpu().tolist()
    return " ".join(str(x) for x in runs)


def rle_decode(rle_str, shape, dtype, device=None):
    """The mask of ``shape`` (``[H, W]``) that ``rle_str`` encodes: 1 where some run covers the pixel, in numpy ``dtype``.  Runs may
    overlap and come in any order.  With a ``device`` the result is a tensor on it (``rle_decode_device``; ``dtype`` may then be numpy's or
    torch's bool / uint8); without one the decode stays on the host, like the reference."""
    if device is not None:
        tdtype = dtype if isinstance(dtype, torch.dtype) else {np.dtype(np.bool_): torch.bool, np.dtype(np.uint8): torch.uint8}.get(np.dtype(dtype), dtype)
        return rle_decode_device(rle_str, shape, dtype=tdtype, device=device)
    runs = _host_runs(rle_str)
    n = int(np.prod(shape))
    pairs = runs.shape[0] // 2
    return _fill_host(runs[0:2 * pairs:2], runs[1:2 * pairs:2], n).astype(dtype).reshape(tuple(shape)[::-1]).T


# ---------------------------------------------------------------------------------------------------------------- host helpers
def _host_runs(runs) -> np.ndarray:
    if isinstance(runs, str):
        return np.array([int(t) for t in runs.split()], dtype=np.int64)
    if isinstance(runs, torch.Tensor):
        runs = runs.detach().cpu().numpy()
    return np.asarray(runs).astype(np.int64, copy=False).reshape(-1)


def _fill_host(starts, lengths, n) -> np.ndarray:
    """uint8[n]: 1 where some run covers the position (runs clipped to 0..n)."""
    lo = np.clip(starts - 1, 0, n)
    hi = np.clip(lo + np.maximum(lengths, 0), lo, n)
    step = np.bincount(lo, minlength=n + 1).astype(np.int64) - np.bincount(hi, minlength=n + 1)
    return (np.cumsum(step)[:n] > 0).astype(np.uint8)


def _encode_host(fg: torch.Tensor) -> torch.Tensor:
    """The encoding of a boolean CPU ``[H, W]`` foreground map, by torch ops."""
    f = fg.t().reshape(-1)
    padded = torch.zeros(f.numel() + 2, dtype=torch.bool)
    padded[1:-1] = f
    edges = torch.nonzero(padded[1:] != padded[:-1]).reshape(-1) + 1
    edges[1::2] -= edges[0::2]
    return edges


def _label_list(labels):
    out = []
    for c in labels:
        if isinstance(c, torch.Tensor) and c.dim() == 0 and not c.is_floating_point() and not c.is_complex() and c.dtype != torch.bool:
            c = int(c.item())
        if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)):
            raise ValueError(f"rle_encode_device: labels must be integers, got {c!r}")
        c = int(c)
        if not -(1 << 63) <= c < (1 << 63):
            raise ValueError(f"rle_encode_device: label {c} does not fit int64")
        out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------- device codec
def rle_encode_device(mask: torch.Tensor, labels=None):
    """Run-length encode ``mask`` on its device.

    ``mask``: ``[H, W]``, or a stack ``[B, H, W]`` whose slices are encoded independently (the z-slices of a label volume); ``bool``,
    ``uint8``, ``int16``, ``int32`` or ``int64``.  ``labels=None``: foreground is ``mask != 0``; ``labels=[c0, c1, ...]``: one encoding
    per label with foreground ``mask == c``, all in the same launches.  Returns one ``int64`` tensor (2-D, no labels), a list with one
    tensor per label (2-D, labels) or per slice (3-D), or a list per slice of lists per label; the tensors are views of one allocation
    on the mask's device, an encoding without foreground is an empty tensor.

    On a CUDA mask the kernels read the mask where it lies (no transposed, boolean or per-label copy), in two phases around ONE read
    of ``8 * (encodings + 1)`` bytes by the host, which sizes the output -- the price ``torch.nonzero`` pays once per call."""
    if not isinstance(mask, torch.Tensor):
        raise TypeError("rle_encode_device: mask must be a tensor (rle_encode takes numpy arrays)")
    if mask.dim() not in (2, 3):
        raise ValueError(f"rle_encode_device: mask must be [H, W] or [B, H, W], got {tuple(mask.shape)}")
    if mask.dtype not in M.ELEM_BYTES:
        raise NotImplementedError(f"rle_encode_device: mask dtype {mask.dtype} (bool, uint8, int16, int32 and int64 are encoded)")
    label_list = None if labels is None else _label_list(labels)
    stack = mask if mask.dim() == 3 else mask[None]
    B, H, W = stack.shape
    K = 0 if label_list is None else len(label_list)
    if B == 0 or H == 0 or W == 0 or (label_list is not None and K == 0):
        flat = [[torch.empty(0, dtype=torch.int64, device=mask.device) for _ in range(1 if label_list is None else K)] for _ in range(B)]
    elif mask.is_cuda:
        flat = _encode_native(stack.contiguous(), label_list)
    else:
        flat = []
        for b in range(B):
            fgs = [stack[b] != 0] if label_list is None else [stack[b] == c if M.fits(c, mask.dtype) else torch.zeros((H, W), dtype=torch.bool) for c in label_list]
            flat.append([_encode_host(fg) for fg in fgs])
    per_slice = [row[0] for row in flat] if label_list is None else flat
    return per_slice if mask.dim() == 3 else per_slice[0]


def _encode_native(stack, label_list):
    B, H, W = stack.shape
    K = 0 if label_list is None else len(label_list)
    E = B * max(K, 1)
    nbytes = N.load().ptb_rle_workspace_bytes(B, K, H, W)
    if nbytes < 0:
        N.check(int(nbytes), "rle_encode_device")
    dev = stack.device
    eb = M.ELEM_BYTES[stack.dtype]
    lab = N.i64_array(label_list) if K else None
    ws = M.scratch(nbytes, dev)
    N.launch("ptb_rle_count", dev, stack.data_ptr(), eb, B, H, W, lab, K, ws.data_ptr(), nbytes, what="rle_encode_device (count)")
    enc = ws[:8 * (E + 1)].view(torch.int64).cpu().tolist()          # the one D2H read: where every encoding starts, and the total
    total = enc[E]
    out = torch.empty(total, dtype=torch.int64, device=dev)
    if total:
        N.launch("ptb_rle_write", dev, stack.data_ptr(), eb, B, H, W, lab, K, ws.data_ptr(), nbytes, out.data_ptr(), total,
                 what="rle_encode_device (write)")
    Kt = max(K, 1)
    views = out.split([enc[e + 1] - enc[e] for e in range(E)])         # (one call: thousands of slice expressions cost milliseconds)
    return [list(views[b * Kt:(b + 1) * Kt]) for b in range(B)]


def rle_decode_device(runs, shape, dtype=torch.uint8, device=None):
    """The ``[H, W]`` mask of ``dtype`` (``torch.bool`` or ``torch.uint8``) holding 1 where some run covers the pixel.

    ``runs``: a string, a sequence, an ndarray or a tensor of ``start, length`` pairs (``start`` is 1-based, column-major); runs may
    overlap and come in any order.  ``device``: where the mask is built; default: the device of a tensor ``runs``, else the CPU.
    Runs given on the host are validated there: an odd count, ``start < 1``, ``length < 0`` or ``start - 1 + length > H * W`` raises
    ``ValueError``.  Runs already on the device are NOT read back: the kernel clamps them to the mask, so nothing is stored out of
    bounds, but the result for runs that violate those rules is unspecified."""
    if dtype not in _DECODE_DTYPES:
        raise NotImplementedError(f"rle_decode_device: dtype {dtype} (torch.bool and torch.uint8 are decoded)")
    if len(shape) != 2:
        raise ValueError(f"rle_decode_device: shape must be (H, W), got {tuple(shape)}")
    H, W = int(shape[0]), int(shape[1])
    if H < 0 or W < 0:
        raise ValueError(f"rle_decode_device: shape must be (H, W), got {tuple(shape)}")
    on_device = isinstance(runs, torch.Tensor) and runs.is_cuda
    device = torch.device(device) if device is not None else (runs.device if isinstance(runs, torch.Tensor) else torch.device("cpu"))
    n = H * W
    if on_device and device.type == "cuda":
        if runs.numel() % 2:
            raise ValueError(f"rle_decode_device: {runs.numel()} values are not (start, length) pairs")
        dev_runs = runs.reshape(-1).to(device=device, dtype=torch.int64).contiguous()
        if dev_runs.data_ptr() % 16:          # (a view that starts in the middle of a pair's 16 bytes: the kernel loads pairs whole)
            dev_runs = dev_runs.clone()
    else:
        host = _host_runs(runs)
        if host.shape[0] % 2:
            raise ValueError(f"rle_decode_device: {host.shape[0]} values are not (start, length) pairs")
        starts, lengths = host[0::2], host[1::2]
        if host.shape[0] and (starts.min() < 1 or lengths.min() < 0 or (starts - 1 + lengths).max() > n):
            raise ValueError(f"rle_decode_device: a run lies outside the {H} x {W} mask (start >= 1, length >= 0, start - 1 + length <= H * W)")
        if device.type != "cuda":
            return torch.from_numpy(_fill_host(starts, lengths, n).reshape(W, H).T.copy()).to(dtype)
        dev_runs = torch.from_numpy(np.ascontiguousarray(host)).to(device)
    mask = torch.empty((H, W), dtype=torch.uint8, device=device)
    if n == 0:
        return mask.to(dtype)
    nbytes = N.load().ptb_rle_decode_workspace_bytes(H, W)
    if nbytes < 0:
        N.check(int(nbytes), "rle_decode_device")
    ws = M.scratch(nbytes, device)
    N.launch("ptb_rle_decode", device, dev_runs.data_ptr(), dev_runs.numel() // 2, H, W, mask.data_ptr(), ws.data_ptr(), nbytes, what="rle_decode_device")
    return mask.view(torch.bool) if dtype == torch.bool else mask
