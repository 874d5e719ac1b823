"""Shapes, inputs and window arithmetic shared by the resize / multiscale sweeps (tests/test_resample_oracle_cpu.py,
tests/test_resample_sweep_gpu.py)."""
from fractions import Fraction

import numpy as np

from oracle import resample_oracle as RO
from oracle import tta_oracle as AO

# (mode, align_corners) of every single-resize kernel
MODE_CASES = [("bilinear", False), ("bilinear", True), ("bicubic", False), ("bicubic", True), ("nearest", None), ("nearest-exact", None), ("area", None)]
MODE_IDS = [m if ac is None else f"{m}-ac{int(ac)}" for m, ac in MODE_CASES]

PLANES = (2, 3)
# (h, w) -> (h', w'): 1-pixel inputs and outputs (align_corners scale 0), ratios 3 and 1/3 (area windows 3 x 3, bicubic clamping on both
# sides), ratios that are no multiple of anything, width 257 (wout % 4 = 1), a transposing aspect change, and a nearest-exact tie (2 -> 141)
SHAPES = [((1, 1), (5, 7)), ((5, 7), (1, 1)), ((5, 7), (1, 9)), ((24, 36), (72, 108)), ((72, 108), (24, 36)), ((65, 100), (63, 257)),
          ((37, 53), (36, 55)), ((13, 300), (300, 13)), ((2, 3), (141, 3))]
SHAPE_IDS = ["%dx%d-%dx%d" % (a + b) for a, b in SHAPES]

# One grid pass is 256 * 32 workgroups of 256 threads = 2 097 152 threads; resize_bilinear_kernel writes 4 outputs per thread, every other
# kernel one.  planes, (h, w) -> (h', w') with just over one pass of outputs: 8 * 1024 * 258 = 2 113 536 threads, 3 * 840 * 1000 = 2 520 000.
GRID_PASS = 256 * 32 * 256
GRID_STRIDE = {"bilinear": ((2, 4), (365, 517), (1024, 1032)), "other": ((1, 3), (300, 357), (840, 1000))}


def grid_stride_case(mode):
    planes, src, dst = GRID_STRIDE["bilinear" if mode == "bilinear" else "other"]
    per_thread = 4 if mode == "bilinear" else 1
    assert planes[0] * planes[1] * dst[0] * ((dst[1] + per_thread - 1) // per_thread) > GRID_PASS
    return planes, src, dst


def uniform(shape, seed, lo=0.05, hi=0.95):
    return (np.random.default_rng(seed).random(shape, dtype=np.float32) * np.float32(hi - lo) + np.float32(lo)).astype(np.float32)


def grad_weights(shape):
    """Upstream gradient of the golden gradient cases: arange % 5 + 1."""
    return (np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape) % 5 + 1).astype(np.float32)


def restated_resize_f32(x, size, mode, align_corners):
    """The float32 numpy restatement of F.interpolate (oracle.tta_oracle); area through the vectorised form of the same sums."""
    if mode == "area":
        return RO.area_resize_f32(x, size)
    return AO._resize(x, size, mode, align_corners)


# ------------------------------------------------------------------------------------------------- nearest-exact ties
def nearest_exact_tie_pairs(limit=300):
    """(n_in, n_out) in 1..limit where the float32 rule floorf((dst + 0.5f) * scale) and the exact rational rule select different
    pixels, found with fractions.Fraction -> {pair: positions}.  Every such position is an exact tie (the rational source coordinate
    is an integer k) where the float32 scale is below n_in / n_out and the product stays below k: the float32 rule takes pixel k - 1
    (asserted here, so users of the set can rely on it)."""
    pairs = {}
    for n_in in range(1, limit + 1):
        for n_out in range(1, limit + 1):
            f32 = RO.nearest_index(n_in, n_out, True, np.float32)
            # integer screen first, then the Fraction statement of the same rule at the positions that differ
            pos = np.nonzero(f32 != RO.nearest_exact_index_rational(n_in, n_out))[0]
            for d in pos:
                coord = Fraction(2 * int(d) + 1, 2) * Fraction(n_in, n_out)
                assert coord.denominator == 1 and f32[d] == coord - 1, (n_in, n_out, d)
            if len(pos):
                pairs[(n_in, n_out)] = [int(d) for d in pos]
    return pairs


# ------------------------------------------------------------------------------------------------- multiscale merge cases
MS_OUT_SIZES = [(72, 136), (71, 135), (70, 137), (69, 134)]          # widths mod 4 = 0, 3, 1, 2; > 1 tile on both axes of every tile shape


def _scaled(size, ry, rx):
    return (max(1, int(round(size[0] * ry))), max(1, int(round(size[1] * rx))))


def ms_source_sets(size):
    """name -> list of source (h, w); every set but ``one_resized`` holds the output size itself once."""
    H, W = size
    sets = {
        "half_one_three": [_scaled(size, 0.5, 0.5), size, _scaled(size, 3, 3)],         # un-staged (ratio 3) next to staged scales
        "rows_1p5": [_scaled(size, 1.5, 1), size],
        "cols_1p5": [_scaled(size, 1, 1.5), size],
        "one_same": [size],
        "one_resized": [((H * 5 // 4) // 4 * 4, (W * 5 // 4) // 4 * 4)],
        "eight": [_scaled(size, r, r) for r in (0.5, 0.75, 0.9)] + [size] + [_scaled(size, r, r) for r in (1.1, 1.25, 1.5, 2.0)],
        "mild_mult4": [((H * 3 // 4) // 4 * 4, (W * 3 // 4) // 4 * 4), size, ((H * 5 // 4) // 4 * 4, (W * 5 // 4) // 4 * 4)],
        "odd_widths": [(H * 3 // 4, (W * 3 // 4) | 1), size, (H * 5 // 4, (W * 5 // 4) // 4 * 4 + 2)],
    }
    return sets


def offsets_for(sources, size):
    """size_offsets of ms_image_deaugment that bring every source back to ``size`` at stride 1."""
    return [0 if tuple(s) == tuple(size) else (s[0] - size[0], s[1] - size[1]) for s in sources]


# ------------------------------------------------------------------------------------------------- source windows of the tiled kernels
def window_extent(n_in, n_out, align_corners, tile, align4=False):
    """Largest number of source rows (columns, with the start rounded down to a multiple of 4 when ``align4``) that the bilinear taps of
    one ``tile``-wide run of outputs span, with the kernels' float32 taps."""
    i0, i1, _ = AO._axis_taps(n_in, n_out, align_corners, np.float32)
    best = 0
    for o0 in range(0, n_out, tile):
        o1 = min(o0 + tile, n_out) - 1
        lo = int(i0[o0]) & ~3 if align4 else int(i0[o0])
        best = max(best, int(i1[o1]) - lo + 1)
    return best
