"""Cases and the two models of the 3-D resampling tests (test_volume_resample_cpu.py, test_volume_resample_gpu.py).

The float64 model: ``oracle.resample_oracle.axis_matrix("bilinear", n_in, n_out, align_corners)`` -- float32 taps in float64 arithmetic,
the model of the 2-D sweep -- applied along z, y and x.  Next to it the float32 numpy restatement of the kernel: the taps of
``oracle.tta_oracle._axis_taps(..., np.float32)``, blended x first, then y, then z, ``a * (1 - l) + b * l`` with every product and sum
rounded to float32.  With d the largest deviation of the restatement from the model on the same input, the kernel stays within
``tol = 4 d + 1e-7`` (the margin allows another summation order); half outputs add the half-ulp of the output type."""
import numpy as np
import torch

from oracle import resample_oracle as RO
from oracle import tta_oracle as AO

# (volume extent, size, what it exercises); every case runs with align_corners both ways
CASES = [
    ((1, 1, 1), (3, 5, 7), "1-voxel source"),
    ((5, 6, 7), (1, 1, 1), "align_corners scale 0"),
    ((12, 18, 21), (18, 27, 32), "the 1.5x case; several bricks along y and z"),
    ((18, 18, 24), (12, 12, 16), "down-sampling"),
    ((4, 5, 6), (12, 15, 18), "ratio 3"),
    ((6, 18, 10), (17, 13, 33), "up and down mixed per axis"),
    ((2, 3, 2), (141, 3, 5), "extreme ratio"),
    ((9, 10, 11), (9, 10, 31), "only one axis resized; the lambda = 0 taps are still multiplied"),
    ((7, 9, 130), (7, 9, 257), "RW % 4 == 1 and a row that spans several 64-element bricks"),
    ((4, 8, 80), (4, 4, 40), "80 x 8 x 4 source voxels under one 64 x 4 x 4 output brick: exactly the LDS brick"),
    ((4, 8, 81), (4, 4, 40), "81 x 8 x 4: the launch gathers from global memory"),
]
CASE_IDS = ["%dx%dx%d-to-%dx%dx%d" % (w + s) for w, s, _ in CASES]
BRICK_FLOATS = 2560                                   # VR_BRICK of csrc/ptb_volume_resample.hip
BRICK_FITS, BRICK_EXCEEDS = CASES[9][:2], CASES[10][:2]


def model_f64(q, size, align_corners):
    """The float64 operator on float32 values ``q`` [C, d, h, w] -> [C, *size]."""
    Rz, Ry, Rx = (RO.axis_matrix("bilinear", q.shape[1 + a], size[a], align_corners) for a in range(3))
    return np.einsum("Zz,Yy,Xx,czyx->cZYX", Rz, Ry, Rx, q.astype(np.float64), optimize=True)


def restated_f32(q, size, align_corners):
    """The kernel's arithmetic in float32 numpy: x, then y, then z."""
    x = np.asarray(q, dtype=np.float32)
    for axis in (3, 2, 1):
        i0, i1, lam = AO._axis_taps(x.shape[axis], size[axis - 1], align_corners, np.float32)
        shape = [1, 1, 1, 1]
        shape[axis] = -1
        x = np.take(x, i0, axis=axis) * (np.float32(1) - lam).reshape(shape) + np.take(x, i1, axis=axis) * lam.reshape(shape)
        assert x.dtype == np.float32
    return x


def tolerance(q, size, align_corners):
    """(model, d, tol) of a case."""
    model = model_f64(q, size, align_corners)
    d = float(np.abs(restated_f32(q, size, align_corners).astype(np.float64) - model).max())
    return model, d, 4 * d + 1e-7


HALF_ULP = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def within(got, model, tol, dtype=torch.float32):
    """Every element of ``got`` (float64 ndarray of the kernel's output in ``dtype``) is within tol + half an ulp of ``dtype`` at the model's
    value.  A float16 output may be infinite where the model reaches the type's overflow threshold, 65520."""
    err = np.abs(got - model)
    ok = err <= tol + HALF_ULP[dtype] * np.abs(model)
    if dtype == torch.float16:
        ok |= np.isinf(got) & (np.sign(got) == np.sign(model)) & (np.abs(model) + tol >= 65520.0)
    return bool(ok.all()), float(np.where(np.isfinite(err), err, 0.0).max())


def volume(dtype, shape, seed):
    """A seeded volume: integer types drawn over the type's full range, float types N(0, 2)."""
    g = torch.Generator().manual_seed(seed)
    if dtype in (torch.uint8, torch.int16, torch.uint16):
        lo, hi = {torch.uint8: (0, 256), torch.int16: (-32768, 32768), torch.uint16: (0, 65536)}[dtype]
        return torch.randint(lo, hi, shape, generator=g, dtype=torch.int32).to(dtype)
    return (torch.randn(shape, generator=g) * 2).to(dtype)


def brick_floats(extent, size, align_corners, channels=1):
    """Source voxels (x channels) under the largest 64 x 4 x 4 output brick of a call: what decides between the LDS-staged launch
    (<= BRICK_FLOATS) and the direct gathers."""
    total = 1
    for n_in, n_out, tile, xc in ((extent[0], size[0], 4, 1), (extent[1], size[1], 4, 1), (extent[2], size[2], 64, channels)):
        i0, i1, _ = AO._axis_taps(n_in, n_out, align_corners, np.float32)
        ne = n_out * xc
        widest = max(int(i1[(min(e0 + tile, ne) - 1) // xc] - i0[e0 // xc] + 1) for e0 in range(0, ne, tile))
        total *= widest * xc
    return total
