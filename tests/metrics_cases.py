"""Shared cases of the confusion-matrix tests and the yardstick they are compared with: a plain restatement of the definition in
numpy (``np.bincount`` over the positions that count, ``np.argmax`` with the first maximum winning and NaN as the maximum) plus a
Python loop for the tiny hand-written matrices.  The reference has no metrics module, so there are no golden vectors; counts are
integers and every comparison is exact."""
import numpy as np

# the work item of csrc/ptb_confusion.hip for a uint8 / uint8 pair: a lane owns LANE_RUN consecutive positions per trip (one 16-byte
# load), a workgroup's 256 lanes own CHUNK, and gridDim.x is at most 8 workgroups per CU (K <= 71: 20 KiB of LDS or less)
LANE_RUN, CHUNK, WGS_256_CU = 16, 4096, 256 * 8
SECOND_TRIP = WGS_256_CU * CHUNK + 3

LENGTHS = [0, 1, 15, 16, 17, LANE_RUN - 1, LANE_RUN + 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, SECOND_TRIP]
# ptb_confusion_plan: the matrix is cut into blocks of floor(16384 / K) target rows; K <= 128 is one block (one read of the maps),
# 129 .. 180 two, 181 .. 221 three, 222 .. 256 four.  Both sides of every boundary, small counts, a prime, and 64 | 65.
ROW_BLOCKS = {128: 1, 129: 2, 180: 2, 181: 3, 221: 3, 222: 4, 256: 4}
CLASS_COUNTS = [1, 2, 4, 19, 64, 65, 128, 129, 150, 180, 181, 221, 222, 256]
NP_DTYPES = {"bool": np.bool_, "u8": np.uint8, "i16": np.int16, "i32": np.int32, "i64": np.int64}
DTYPE_PAIRS = [("u8", "u8"), ("u8", "i64"), ("i64", "u8"), ("i64", "i64"), ("i16", "u8"), ("u8", "i32"), ("i32", "i16")]
CONTENTS = ("constant", "blobs", "noise", "aligned_runs")


def make_map(content, n, K, seed):
    """int64[n] labels in [0, K), a function of the arguments only."""
    rng = np.random.default_rng(seed)
    if content == "constant":                                   # one cell: every lane of every wave adds to the same counter
        return np.full(n, K - 1, np.int64)
    if content == "noise":
        return rng.integers(0, K, n).astype(np.int64)
    if content == "blobs":                                      # long runs of random length
        runs = rng.integers(1, 700, n // 200 + 2)
        return np.repeat(rng.integers(0, K, runs.shape[0]), runs)[:n].astype(np.int64) if n else np.zeros(0, np.int64)
    if content == "aligned_runs":                               # runs that end exactly where a lane's run, a load and a chunk end
        i = np.arange(n)
        return ((i // LANE_RUN) + (i // CHUNK)) % K
    raise ValueError(content)


def make_pair(content, n, K, seed, pred_dtype="u8", target_dtype="u8"):
    """(pred, target) numpy arrays: the target by ``content``, the pred the target with one position in five relabelled."""
    t = make_map(content, n, K, seed)
    rng = np.random.default_rng(seed + 1000)
    p = np.where(rng.random(n) < 0.2, rng.integers(0, K, n), t)
    return p.astype(NP_DTYPES[pred_dtype]), t.astype(NP_DTYPES[target_dtype])


def restate_loop(pred, target, K, ignore_index=None):
    """The definition, position by position: (matrix, invalid)."""
    cm = [[0] * K for _ in range(K)]
    invalid = 0
    for p, t in zip(np.asarray(pred).reshape(-1).tolist(), np.asarray(target).reshape(-1).tolist()):
        p, t = int(p), int(t)
        if ignore_index is not None and t == ignore_index:
            continue
        if not (0 <= t < K and 0 <= p < K):
            invalid += 1
            continue
        cm[t][p] += 1
    return np.array(cm, np.int64).reshape(K, K), invalid


def restate(pred, target, K, ignore_index=None, per_sample=False):
    """(int64 [K, K] or [B, K, K], invalid) by ``np.bincount``."""
    pred, target = np.asarray(pred), np.asarray(target)
    if per_sample:
        parts = [restate(pred[b], target[b], K, ignore_index) for b in range(pred.shape[0])]
        return np.stack([c for c, _ in parts]).reshape(-1, K, K), sum(i for _, i in parts)
    p, t = pred.reshape(-1).astype(np.int64), target.reshape(-1).astype(np.int64)
    live = np.ones(t.shape, bool) if ignore_index is None else t != ignore_index
    inside = (t >= 0) & (t < K) & (p >= 0) & (p < K)
    keep = live & inside
    return np.bincount(t[keep] * K + p[keep], minlength=K * K).astype(np.int64).reshape(K, K), int((live & ~inside).sum())


def restate_argmax(logits, threshold=0.0):
    """The prediction of float32 ``[N, C, *S]`` logits: ``np.argmax`` -- first occurrence of the maximum, a NaN being the maximum."""
    x = np.asarray(logits, np.float32)
    if x.shape[1] == 1:
        return (x[:, 0] > np.float32(threshold)).astype(np.int64)
    nan = np.isnan(x)
    first_nan = np.argmax(nan, axis=1)
    plain = np.argmax(np.where(nan, -np.inf, x), axis=1)
    return np.where(nan.any(axis=1), first_nan, plain).astype(np.int64)


def restate_scores(cm):
    cm = np.asarray(cm).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        tp = np.diagonal(cm, axis1=-2, axis2=-1)
        fp, fn = cm.sum(-2) - tp, cm.sum(-1) - tp
        iou, dice = tp / (tp + fp + fn), (2 * tp) / (2 * tp + fp + fn)

        def nanmean(x):
            ok = ~np.isnan(x)
            return np.where(ok, x, 0.0).sum(-1) / ok.sum(-1)

        return {"iou": iou, "dice": dice, "precision": tp / (tp + fp), "recall": tp / (tp + fn), "accuracy": tp.sum(-1) / cm.sum((-2, -1)),
                "mean_iou": nanmean(iou), "mean_dice": nanmean(dice)}


# ---- the label cases both files walk: (name, n, K, pred dtype, target dtype, content, ignore_index, hostile) -------------------------
def label_cases():
    cases = []
    for n in LENGTHS:
        cases.append((f"len{n}", n, 4, "u8", "u8", "blobs", None, False))
    for K in CLASS_COUNTS:
        wide = "i16" if K > 200 else "u8"                        # (room for values >= K)
        cases.append((f"K{K}", 3 * CHUNK + 5, K, wide, wide, "noise", None, True))
    for pd, td in DTYPE_PAIRS:
        cases.append((f"{pd}-{td}", 2 * CHUNK + 17, 6, pd, td, "blobs", None, True))
    cases.append(("bool-bool", 2 * CHUNK + 17, 2, "bool", "bool", "noise", None, False))
    for content in CONTENTS:
        cases.append((content, 5 * CHUNK + 33, 5, "u8", "u8", content, None, False))
    cases.append(("ignore255", 2 * CHUNK + 9, 4, "u8", "u8", "blobs", 255, True))
    cases.append(("ignore-100", 2 * CHUNK + 9, 4, "i64", "i64", "blobs", -100, True))
    cases.append(("ignore0", 2 * CHUNK + 9, 4, "u8", "i64", "noise", 0, True))
    return cases


def build_case(case):
    """(pred, target) of a case.  ``hostile``: positions with values outside [0, K) in either map (negatives where the type has them,
    255 in uint8) and positions holding the ignore value."""
    name, n, K, pd, td, content, ignore, hostile = case
    p, t = make_pair(content, n, K, abs(hash_name(name)) % 10000, pd, td)
    if hostile and n:
        rng = np.random.default_rng(n + K)
        for arr, dt in ((p, pd), (t, td)):
            if dt == "bool":
                continue
            where = rng.integers(0, n, max(1, n // 50))
            hi = min(np.iinfo(arr.dtype).max, K + 70)
            vals = rng.integers(K, hi + 1, where.shape[0]) if hi >= K else np.zeros(where.shape[0], np.int64)
            if np.iinfo(arr.dtype).min < 0:
                vals = np.where(rng.random(where.shape[0]) < 0.5, -1 - vals, vals)
            elif K <= 255:
                vals[::3] = 255
            if hi >= K or np.iinfo(arr.dtype).min < 0:
                arr[where] = vals.astype(arr.dtype)
        if ignore is not None and NP_DTYPES[td] is not np.bool_ and np.iinfo(t.dtype).min <= ignore <= np.iinfo(t.dtype).max:
            t[rng.integers(0, n, max(1, n // 20))] = ignore
    return p, t


def hash_name(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))
