"""GPU: the confusion-matrix kernels (csrc/ptb_confusion.hip) equal the restatement of tests/metrics_cases.py exactly -- these are
integer counts -- over the shapes at which the kernels change path.

Dispatch boundaries of the implementation (ptb_confusion_plan; metrics_cases.ROW_BLOCKS):
  * K <= 128: the whole matrix is one LDS histogram; 129 .. 180: two row blocks (the maps are read twice), 181 .. 221: three,
    222 .. 256: four.  K = 128 | 129, 180 | 181, 221 | 222 are all in metrics_cases.CLASS_COUNTS.
  * a chunk (256 lanes x one lane run) that lies whole inside its sample and whose sample bases are 16-byte aligned takes the wide
    loads, every other chunk the element-wise body: lengths around one lane run and one chunk, views offset by one element, and
    per-sample bases of 1001 positions.
  * the workgroups of one launch are capped at 8 per CU (K <= 71), so metrics_cases.SECOND_TRIP positions make the grid-stride loop
    take a second trip on a 256-CU device."""
import ctypes

import numpy as np
import pytest
import torch

import metrics_cases as MC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import metrics as M

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _cm(pred, target, K, **kw):
    before = N.calls
    got = M.confusion_matrix(pred, target, K, **kw)
    assert N.calls == before + 1, "one native call per confusion matrix"
    assert got.dtype == torch.int64 and got.device == DEV
    return got


def _logits(x, t, **kw):
    before = N.calls
    got = M.confusion_matrix_from_logits(x, t, **kw)
    assert N.calls == before + 1, "one native call per confusion matrix"
    assert got.dtype == torch.int64 and got.device == DEV
    return got


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def test_plan_matches_the_documented_boundaries():
    lib = N.load()
    for K in range(1, 257):
        rb, lds = ctypes.c_int(), ctypes.c_int()
        assert lib.ptb_confusion_plan(K, ctypes.byref(rb), ctypes.byref(lds)) == 0
        rows = min(K, 16384 // K)
        assert rb.value == -(-K // rows) and lds.value == rows * K * 4 <= 64 * 1024
        if K in MC.ROW_BLOCKS:
            assert rb.value == MC.ROW_BLOCKS[K]
    assert lib.ptb_confusion_plan(257, None, None) == N.PTB_EUNSUPPORTED and lib.ptb_confusion_plan(0, None, None) == -1


@pytest.mark.parametrize("case", MC.label_cases(), ids=lambda c: c[0])
def test_label_cases(case):
    name, n, K, pd, td, content, ignore, hostile = case
    p, t = MC.build_case(case)
    want, invalid = MC.restate(p, t, K, ignore)
    dp, dt = _dev(p), _dev(t)
    if n == 0:
        before = N.calls
        got = M.confusion_matrix(dp, dt, K, ignore_index=ignore)
        assert N.calls == before, "an empty input launches nothing"
    else:
        got = _cm(dp, dt, K, ignore_index=ignore)                  # strict=False skips what is out of range
    assert got.shape == (K, K) and np.array_equal(got.cpu().numpy(), want)
    if invalid:
        with pytest.raises(ValueError, match=rf"\b{invalid} position"):
            M.confusion_matrix(dp, dt, K, ignore_index=ignore, strict=True)
    elif n:
        assert torch.equal(_cm(dp, dt, K, ignore_index=ignore, strict=True), got)


@pytest.mark.parametrize("which", ["pred", "target", "both"])
def test_base_pointer_offset_by_one_element(which):
    for pd, td in (("u8", "u8"), ("i64", "u8"), ("u8", "i64")):
        n, K = 2 * MC.CHUNK + 17, 5
        p, t = MC.make_pair("blobs", n, K, 11, pd, td)
        want, _ = MC.restate(p, t, K)
        dp, dt = _dev(p), _dev(t)
        if which in ("pred", "both"):
            buf = torch.zeros(n + 1, dtype=dp.dtype, device=DEV)
            buf[1:] = dp
            dp = buf[1:]
            assert dp.is_contiguous() and dp.data_ptr() % 16 != 0
        if which in ("target", "both"):
            buf2 = torch.zeros(n + 1, dtype=dt.dtype, device=DEV)
            buf2[1:] = dt
            dt = buf2[1:]
            assert dt.is_contiguous() and dt.data_ptr() % 16 != 0
        assert np.array_equal(_cm(dp, dt, K).cpu().numpy(), want), (which, pd, td)


def test_out_of_range_values_touch_nothing_else():
    """Hostile maps (negatives, values >= K, 255 in uint8 with K = 4) with the result inside a guarded allocation."""
    n, K = 3 * MC.CHUNK + 5, 4
    for pd, td in (("u8", "u8"), ("i64", "i64"), ("i64", "u8")):
        rng = np.random.default_rng(17)
        p, t = MC.make_pair("noise", n, K, 13, pd, td)
        for arr in (p, t):
            where = rng.integers(0, n, n // 3)
            lo = -(2 ** 62) if arr.dtype == np.int64 else 0
            hi = 2 ** 62 if arr.dtype == np.int64 else 255
            arr[where] = rng.integers(lo, hi, where.shape[0], endpoint=True).astype(arr.dtype)
            arr[where[::5]] = 255 if arr.dtype == np.uint8 else -1
        want, invalid = MC.restate(p, t, K)
        assert invalid > n // 4
        guard = torch.full((3, K, K), 0x5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
        guard[1] = 0
        got = _cm(_dev(p), _dev(t), K, out=guard[1])
        assert got.data_ptr() == guard[1].data_ptr() and np.array_equal(guard[1].cpu().numpy(), want)
        assert bool((guard[0] == 0x5A5A5A5A5A5A).all()) and bool((guard[2] == 0x5A5A5A5A5A5A).all())
        with pytest.raises(ValueError, match=rf"\b{invalid} position"):
            M.confusion_matrix(_dev(p), _dev(t), K, strict=True)


def test_per_sample():
    K = 6
    for B, shape in ((3, (7, 143)), (1, (1001,)), (64, (33, 31))):          # 1001 and 1023 positions per sample: odd sample bases
        n = int(np.prod(shape))
        p, t = MC.make_pair("blobs", B * n, K, 23 + B)
        p[::97] = 200                                                        # out of range in some samples
        dp, dt = _dev(p).view(B, *shape), _dev(t).view(B, *shape)
        per = _cm(dp, dt, K, per_sample=True, ignore_index=1)
        want, _ = MC.restate(p.reshape(B, n), t.reshape(B, n), K, 1, per_sample=True)
        assert per.shape == (B, K, K) and np.array_equal(per.cpu().numpy(), want)
        assert torch.equal(per, torch.stack([_cm(dp[b], dt[b], K, ignore_index=1) for b in range(min(B, 4))] + list(per[4:])))
        assert torch.equal(per.sum(0), _cm(dp, dt, K, ignore_index=1))
    # more samples than one launch carries in gridDim.z (65535): the host splits the batch
    B, n = 65535 + 4, 5
    p, t = MC.make_pair("noise", B * n, 3, 37)
    per = _cm(_dev(p).view(B, n), _dev(t).view(B, n), 3, per_sample=True)
    idx = (np.arange(B * n) // n) * 9 + t.astype(np.int64) * 3 + p
    assert np.array_equal(per.cpu().numpy(), np.bincount(idx, minlength=B * 9).reshape(B, 3, 3))
    x = torch.from_numpy(np.random.default_rng(38).standard_normal((B, 2, n)).astype(np.float32))
    per = _logits(x.to(DEV), _dev(t).view(B, n), per_sample=True)
    idx = (np.arange(B * n) // n) * 4 + t.astype(np.int64) * 2 + MC.restate_argmax(x.numpy()).reshape(-1)
    keep = t < 2
    assert np.array_equal(per.cpu().numpy(), np.bincount(idx[keep], minlength=B * 4).reshape(B, 2, 2))
    # a sample count whose bases are aligned again, many classes
    p, t = MC.make_pair("noise", 4 * 8192, 150, 29)
    per = _cm(_dev(p).view(4, 8192), _dev(t).view(4, 8192), 150, per_sample=True)
    assert np.array_equal(per.cpu().numpy(), MC.restate(p.reshape(4, -1), t.reshape(4, -1), 150, per_sample=True)[0])


def test_out_accumulates_in_64_bits_without_a_synchronisation():
    n, K = 3 * MC.CHUNK + 5, 5
    p, t = MC.make_pair("blobs", n, K, 31)
    p2, t2 = MC.make_pair("noise", n, K, 32)
    a, b = MC.restate(p, t, K)[0], MC.restate(p2, t2, K)[0]
    dp, dt, dp2, dt2 = _dev(p), _dev(t), _dev(p2), _dev(t2)
    out = torch.full((K, K), 2 ** 32 - 3, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                  # any synchronising call raises from here on
    try:
        back = _cm(dp, dt, K, out=out)
        _cm(dp2, dt2, K, out=out)
        fresh = _cm(dp, dt, K)
        with pytest.raises(RuntimeError):
            M.confusion_matrix(dp, dt, K, strict=True)                       # the 8-byte read of strict=True is one
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert back is out
    assert np.array_equal(out.cpu().numpy(), a + b + (2 ** 32 - 3)) and int(out.max()) > 2 ** 32
    assert np.array_equal(fresh.cpu().numpy(), a)
    for bad in (torch.zeros((K, K), dtype=torch.int64), torch.zeros((K, K), dtype=torch.int32, device=DEV), torch.zeros((K + 1, K), dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError):
            M.confusion_matrix(dp, dt, K, out=bad)
    with pytest.raises(NotImplementedError, match="bincount"):
        M.confusion_matrix(dp, dt, 257)
    with pytest.raises(ValueError):
        M.confusion_matrix(dp, dt.cpu(), K)
    assert np.array_equal(_cm(dp.view(-1, 19).t(), dt.view(-1, 19).t(), K).cpu().numpy(), a)      # non-contiguous: copied first


# ---------------------------------------------------------------------------------------------------------------- logits
def _crafted_logits(shape, seed):
    """float32 logits with ties, -0.0 against 0.0, NaN in the first / a middle / the last channel, all-NaN positions and infinities."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    x = np.round(x * 4) / 4                                                  # quarter steps: exact in bf16 / fp16, plenty of equal maxima
    N_, C = shape[0], shape[1]
    flat = x.reshape(N_, C, -1)
    S = flat.shape[2]
    idx = np.arange(S)
    flat[:, :, idx % 11 == 0] = 0.0
    flat[:, 0, idx % 22 == 0] = -0.0                                         # -0.0 first, 0.0 behind it: the first wins
    flat[:, 0, idx % 13 == 1] = np.nan
    flat[:, C // 2, idx % 13 == 2] = np.nan
    flat[:, C - 1, idx % 13 == 3] = np.nan
    flat[:, :, idx % 17 == 4] = np.nan
    flat[:, C - 1, idx % 19 == 5] = np.inf
    flat[:, :, idx % 23 == 6] = np.inf                                       # a tie of infinities
    flat[:, :, idx % 29 == 7] = -np.inf
    flat[:, C // 2, idx % 31 == 8] = 3.0
    flat[:, C - 1, idx % 31 == 8] = 3.0                                      # equal maxima: the earlier channel
    return flat.reshape(shape)


LOGIT_SHAPES = [(2, 1, 5, 13), (2, 2, 5, 13), (2, 3, 5, 13), (2, 4, 5, 13), (2, 19, 5, 13), (2, 256, 5, 13), (1, 3, 3, 7, 11), (1, 1, 3, 7, 11), (2, 4, 64, 64),
                (3, 4, 1, 2048 + 8), (1, 19, 48, 128), (2, 150, 8, 256)]
TORCH_DTYPES = {"u8": torch.uint8, "i16": torch.int16, "i32": torch.int32, "i64": torch.int64}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=str)
@pytest.mark.parametrize("shape", LOGIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_logits(shape, dtype):
    x = torch.from_numpy(_crafted_logits(shape, sum(shape))).to(dtype)
    C = shape[1]
    K = max(C, 2)
    thr = 0.25
    pred = MC.restate_argmax(x.float().numpy(), thr)
    rng = np.random.default_rng(sum(shape) + 1)
    tshape = (shape[0],) + shape[2:]
    for td, ignore in (("u8", 255 if K < 256 else None), ("i64", -100), ("i16", None), ("i32", 0)):
        t = rng.integers(0, K, tshape)
        if ignore is not None:
            t[rng.random(tshape) < 0.1] = ignore
        if td != "u8" or K < 200:
            t[rng.random(tshape) < 0.05] = K + 3 if td == "u8" else -7      # out of range
        t = torch.from_numpy(t).to(TORCH_DTYPES[td])
        want, invalid = MC.restate(pred, t.numpy(), K, ignore)
        dx, dt = x.to(DEV), t.to(DEV)
        got = _logits(dx, dt, ignore_index=ignore, threshold=thr)
        assert got.shape == (K, K) and np.array_equal(got.cpu().numpy(), want), (td, ignore)
        assert torch.equal(got, _cm(_dev(pred), dt, K, ignore_index=ignore))
        per = _logits(dx, dt, ignore_index=ignore, threshold=thr, per_sample=True)
        assert per.shape == (shape[0], K, K) and torch.equal(per.sum(0), got)
        assert np.array_equal(per.cpu().numpy(), MC.restate(pred, t.numpy(), K, ignore, per_sample=True)[0])
        if invalid:
            with pytest.raises(ValueError, match=rf"\b{invalid} position"):
                M.confusion_matrix_from_logits(dx, dt, ignore_index=ignore, threshold=thr, strict=True)


def test_logits_layouts_views_and_out():
    x = torch.from_numpy(_crafted_logits((2, 4, 24, 40), 3))
    t = torch.from_numpy(np.random.default_rng(4).integers(0, 4, (2, 24, 40))).to(torch.uint8)
    want, _ = MC.restate(MC.restate_argmax(x.numpy()), t.numpy(), 4)
    dx, dt = x.to(DEV), t.to(DEV)
    cl = dx.contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    assert np.array_equal(_logits(cl, dt).cpu().numpy(), want)               # channels-last: copied to dense first, the same matrix
    x5 = dx.view(2, 4, 2, 12, 40).contiguous(memory_format=torch.channels_last_3d)
    assert not x5.is_contiguous() and np.array_equal(_logits(x5, dt.view(2, 2, 12, 40)).cpu().numpy(), want)
    # odd bases: logits and target one element into their allocations
    for dtype in (torch.float32, torch.bfloat16):
        xd = dx.to(dtype)
        w2, _ = MC.restate(MC.restate_argmax(xd.float().cpu().numpy()), t.numpy(), 4)
        buf = torch.zeros(xd.numel() + 1, dtype=dtype, device=DEV)
        buf[1:] = xd.reshape(-1)
        tb = torch.zeros(dt.numel() + 1, dtype=torch.uint8, device=DEV)
        tb[1:] = dt.reshape(-1)
        assert np.array_equal(_logits(buf[1:].view(xd.shape), dt).cpu().numpy(), w2)
        assert np.array_equal(_logits(xd, tb[1:].view(dt.shape)).cpu().numpy(), w2)
    out = torch.full((4, 4), 2 ** 32 - 3, dtype=torch.int64, device=DEV)
    assert _logits(dx, dt, out=out) is out and np.array_equal(out.cpu().numpy(), want + (2 ** 32 - 3))
    with pytest.raises(NotImplementedError):
        M.confusion_matrix_from_logits(torch.zeros((1, 257, 4), device=DEV), torch.zeros((1, 4), dtype=torch.uint8, device=DEV))
    before = N.calls
    assert int(M.confusion_matrix_from_logits(dx[:0], dt[:0]).sum()) == 0 and N.calls == before


def test_pipeline_merge_crop_argmax_into_scores():
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer, TileMerger

    C, tile, step = 4, 64, 32
    slicer = ImageSlicer((150, 203, 3), tile, step, weight="pyramid")
    g = torch.Generator().manual_seed(71)
    outputs = torch.randn((len(slicer.crops), C, tile, tile), generator=g)
    outputs = torch.nn.functional.avg_pool2d(outputs, 9, stride=1, padding=4)    # smooth logits: regions instead of specks
    merger = TileMerger(slicer.target_shape, C, slicer.weight, device=DEV)
    merger.integrate_batch(outputs.to(DEV), slicer.crops)
    labels_map = merger.merge_crop(slicer, argmax=True, dtype=torch.uint8)
    truth = torch.from_numpy(MC.make_map("blobs", 150 * 203, C, 72).astype(np.uint8)).view(150, 203)
    truth[:10] = 255                                                             # an unlabelled border
    cm = _cm(labels_map, truth.to(DEV), C, ignore_index=255)
    want, invalid = MC.restate(labels_map.cpu().numpy(), truth.numpy(), C, 255)
    assert invalid == 0 and np.array_equal(cm.cpu().numpy(), want) and int(cm.sum()) == 140 * 203
    scores, ref = M.segmentation_scores(cm), MC.restate_scores(want)
    for k in ("iou", "dice", "precision", "recall", "accuracy"):
        assert scores[k].device == DEV and np.array_equal(scores[k].cpu().numpy(), ref[k], equal_nan=True), k
    assert np.allclose(scores["mean_iou"].cpu().numpy(), ref["mean_iou"], rtol=1e-12, atol=0)
