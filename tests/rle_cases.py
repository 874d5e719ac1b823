"""Shared cases of the run-length codec tests: seeded masks by name, the golden's case list (tools/make_rle_golden.py records the
reference's answers for it in tests/golden/rle.npz) and an independent restatement of the encoding -- a plain loop over the
column-major pixel sequence that emits the runs, without the reference's ``np.where`` trick."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rle.npz")

PATTERNS = ("zeros", "ones", "first", "last", "wrap", "checker", "noise", "blobs")

# the work item of csrc/ptb_rle.hip: RLE_COLS columns x RLE_SEG rows per segment, RLE_WY segments per workgroup
SEG_ROWS, ITEM_COLS, GROUP_ROWS = 32, 256, 128

SMALL_SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (37, 53)]
ITEM_SHAPES = [(SEG_ROWS, ITEM_COLS), (SEG_ROWS - 1, ITEM_COLS - 1), (SEG_ROWS + 1, ITEM_COLS + 1),
               (GROUP_ROWS, ITEM_COLS), (GROUP_ROWS - 1, ITEM_COLS + 1), (GROUP_ROWS + 1, ITEM_COLS - 1)]
LARGE_SHAPES = [(129, 257), (300, 77)]
ALL_SHAPES = SMALL_SHAPES + ITEM_SHAPES + LARGE_SHAPES


def make_mask(pattern, shape, seed=0):
    """A uint8 0/1 mask of ``shape`` (``labels6``: a label map with values 0..5), a function of its arguments only."""
    H, W = shape
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), np.uint8)
    if pattern == "zeros":
        pass
    elif pattern == "ones":
        m[:] = 1
    elif pattern == "first":
        m[0, 0] = 1
    elif pattern == "last":
        m[-1, -1] = 1
    elif pattern == "wrap":                     # one run from the bottom of a column into the top of the next one (degenerate shapes: what fits)
        c = max(W // 2 - 1, 0)
        m[max(H - 2, 0):, c] = 1
        if c + 1 < W:
            m[:min(2, H), c + 1] = 1
    elif pattern == "checker":
        yy, xx = np.mgrid[0:H, 0:W]
        m[:] = (yy + xx) & 1
    elif pattern == "noise":
        m[:] = rng.random((H, W)) < 0.5
    elif pattern == "blobs":
        yy, xx = np.mgrid[0:H, 0:W]
        for _ in range(6):
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1, max(2.0, 0.2 * max(H, W)))
            m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    elif pattern == "labels6":
        yy, xx = np.mgrid[0:H, 0:W]
        m[:] = rng.integers(0, 6, ((H + 7) // 8, (W + 7) // 8))[yy // 8, xx // 8]      # 8 x 8 patches of one label ...
        speck = rng.random((H, W)) < 0.1
        m[speck] = rng.integers(0, 6, int(speck.sum()))                                  # ... with single-pixel specks
    else:
        raise ValueError(pattern)
    return m


def _case(pattern, shape, seed=0):
    return {"name": f"{pattern}_{shape[0]}x{shape[1]}_s{seed}", "pattern": pattern, "shape": list(shape), "seed": seed}


# what tools/make_rle_golden.py records (every mask <= 300 x 300; only seeds and parameters are stored)
GOLDEN_CASES = ([_case("zeros", (1, 1)), _case("ones", (1, 1)), _case("noise", (1, 7), 1), _case("noise", (7, 1), 2)]
                + [_case(p, s, 3) for s in [(5, 3), (37, 53), (129, 257), (300, 77)] for p in PATTERNS]
                + [_case("labels6", (37, 53), 4), _case("labels6", (129, 257), 5)])

# decode only: runs that overlap, repeat, touch and come out of order, in a (37, 53) mask
OVERLAP_SHAPE = (37, 53)
OVERLAP_RUNS = [400, 50, 1, 3, 420, 10, 100, 37, 90, 20, 1961, 1, 1200, 0, 3, 5, 400, 50, 1500, 300, 1700, 12]


def case_mask(case):
    return make_mask(case["pattern"], tuple(case["shape"]), case["seed"])


def load_golden():
    z = np.load(GOLDEN, allow_pickle=False)
    return z, json.loads(str(z["__cases__"]))


def restate(fg):
    """The encoding of a boolean [H, W] foreground map straight from its definition: walk p = 0 .. N - 1 over f[p] = fg[p % H][p // H],
    open a run where f turns on, close it where f turns off (or at p = N)."""
    fg = np.asarray(fg) != 0
    H, W = fg.shape
    out, start = [], None
    for p in range(H * W):
        on = bool(fg[p % H, p // H])
        if on and start is None:
            start = p
        elif not on and start is not None:
            out += [start + 1, p - start]
            start = None
    if start is not None:
        out += [start + 1, H * W - start]
    return np.asarray(out, dtype=np.int64)


def restate_fast(fg):
    """``restate`` without the Python loop, for the shapes where that would take seconds (tests/test_rle_cpu.py holds the two equal)."""
    f = np.ascontiguousarray((np.asarray(fg) != 0).T).reshape(-1).astype(np.int8)
    step = np.diff(f, prepend=np.int8(0), append=np.int8(0))
    starts, ends = np.flatnonzero(step == 1), np.flatnonzero(step == -1)
    out = np.empty(2 * starts.shape[0], np.int64)
    out[0::2] = starts + 1
    out[1::2] = ends - starts
    return out


def decode_restate(runs, shape):
    """The mask the runs cover, by the definition's loop (runs may overlap and come in any order)."""
    H, W = shape
    flat = np.zeros(H * W, np.uint8)
    runs = np.asarray(runs, dtype=np.int64).reshape(-1, 2)
    for start, length in runs:
        flat[start - 1:start - 1 + length] = 1
    return flat.reshape(W, H).T.copy()
