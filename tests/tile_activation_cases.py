"""The float64 model of ``activation=`` in the 2-D de-augmentations and tile merges, shared by tests/test_tile_activation_cpu.py and
tests/test_tile_activation_gpu.py -- the 2-D twin of tests/volume_activation_cases.py, whose constants and helpers it reuses.  The chain:
A in float64 on the (already rounded) logits, inverse views, reduce, blend in integration order, divide."""
import numpy as np
import torch

from volume_activation_cases import (ARGMAX_GAP, ARGMAX_SKIP, REDUCTIONS, TOL, activate64, assert_close, logits,  # noqa: F401
                                     reduce64)

from pytorch_toolbelt_amd.inference.tta import DEAUGMENT_VIEWS

GROUPS = ("fliplr", "flipud", "flips", "d2", "d4")
ACTIVATIONS = ("sigmoid", "softmax")
# Temperatures of the cases that are compared with this model stay at or below MAX_TEMPERATURE.  The calls are DEFINED on the float32
# tensor A(y), and "logodd" divides an error eps of a probability by p (1 - p): the result moves by up to 0.25 * eps / (1 - p).  float32
# alone rounds p near 1 by 2^-25; with the one-ulp exp / reciprocal and the channel sum, eps <= 4 ulp = 2.4e-7.  Logits in [-3, 3] at
# temperature t leave 1 - p >= 2 exp(-6 t) for a softmax: 9.0e-3 at t = 0.9, so the bound is 0.25 * 2.4e-7 / 9.0e-3 = 6.7e-6 < TOL; at
# t = 1.3 (8.2e-4) it would be 7e-5, which no float32 evaluation of A(y) followed by "logodd" can meet.
MAX_TEMPERATURE = 0.9


def view64(x, code):
    """View ``code`` (bit 0 transpose, bit 1 flip the source rows, bit 2 flip the source columns; include/ptb_hip.h) of ``[B, C, H, W]``
    in plain torch ops: out[i][j] = src[rr][cc] with (rr, cc) = (j, i) for a transposing view, then mirrored."""
    if code & 2:
        x = x.flip(2)
    if code & 4:
        x = x.flip(3)
    return x.transpose(2, 3) if code & 1 else x


def deaugment64(y, group, reduction, activation, temperature=1.0):
    """``[V*B, C, H, W]`` logits -> float64 ``[B, C, H, W]``; ``group=None``: ``A(y)`` itself."""
    p = activate64(y, activation, temperature)
    if group is None:
        return p
    views = DEAUGMENT_VIEWS[group]
    return reduce64(torch.stack([view64(c, v) for c, v in zip(torch.chunk(p, len(views)), views)]), reduction)


def merge64(slicer, channels, tiles):
    """Blend float64 ``[n, C, h, w]`` tiles at the slicer's crops, in integration order: ``[C, H', W']``, NaN where nobody covers."""
    H, W = slicer.target_shape[:2]
    total = torch.zeros((channels, H, W), dtype=torch.float64)
    mass = torch.zeros((H, W), dtype=torch.float64)
    w = torch.from_numpy(np.asarray(slicer.weight)).double()
    for tile, (x, y, tw, th) in zip(tiles, slicer.crops):
        total[:, y:y + th, x:x + tw] += tile * w
        mass[y:y + th, x:x + tw] += w
    return total / mass


def batches(slicer, channels, group, dtype, bs, seed):
    """The model outputs of a whole image: a list of (chunk-major ``[V*b, C, h, w]`` CPU logits, crops)."""
    views = 1 if group is None else len(DEAUGMENT_VIEWS[group])
    th, tw = slicer.tile_size
    out = []
    for i, b0 in enumerate(range(0, len(slicer.crops), bs)):
        crops = slicer.crops[b0:b0 + bs]
        out.append((logits((views * len(crops), channels, th, tw), dtype, seed * 1000 + i), crops))
    return out


def model_image(slicer, channels, fed, group, reduction, activation, temperature=1.0):
    tiles = torch.cat([deaugment64(y, group, reduction, activation, temperature) for y, _ in fed])
    return merge64(slicer, channels, tiles)


def near_tie_share(want):
    """Share of the covered pixels of float64 ``[C, H, W]`` probabilities whose top-two gap is below ARGMAX_GAP."""
    if want.shape[0] < 2:
        return 0.0
    nan = torch.isnan(want).any(dim=0)
    top = want.nan_to_num(0.0).topk(2, dim=0).values
    return float((((top[0] - top[1]) < ARGMAX_GAP) & ~nan).double().mean())


def assert_argmax(got, want, what):
    """``[H, W]`` labels against the float64 probabilities ``want`` ``[C, H, W]``: near-ties are left out (at most ARGMAX_SKIP of the
    pixels); never-covered pixels are whatever the kernel says."""
    got = got.detach().cpu().long()
    nan = torch.isnan(want).any(dim=0)
    share = near_tie_share(want)
    print(f"{what}: {100 * share:.3f} % of the pixels left out as near-ties")
    assert share <= ARGMAX_SKIP, (what, share)
    keep = ~nan
    if want.shape[0] > 1:
        top = want.nan_to_num(0.0).topk(2, dim=0).values
        keep &= (top[0] - top[1]) >= ARGMAX_GAP
    assert torch.equal(got[keep], want.nan_to_num(0.0).argmax(dim=0)[keep]), what
