"""GPU: the run-length codec's HIP path (csrc/ptb_rle.hip) equals the definition's restatement (tests/rle_cases.py) and the reference's
recorded answers (tests/golden/rle.npz) exactly -- these are integers -- over the shapes at which the kernels change path: degenerate
masks, sizes around the work item (256 columns x 32-row segments, four segments per workgroup), W % 4 != 0 and odd base addresses
(the peeled loads), every element type, labels, stacks, and a count array long enough for every level of the scan."""
import json

import numpy as np
import pytest
import torch

import rle_cases as RC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import rle as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _encode(t, **kw):
    before = N.calls
    got = R.rle_encode_device(t, **kw)
    assert N.calls > before, "the native path did not run"
    return got


def _decode(runs, shape, **kw):
    before = N.calls
    got = R.rle_decode_device(runs, shape, **kw)
    assert N.calls > before, "the native path did not run"
    return got


def _check(m, got):
    """``got`` is the device encoding of the 0/1 host mask ``m``; it also decodes back to ``m``."""
    assert got.dtype == torch.int64 and got.device == DEV and got.dim() == 1
    want = RC.restate_fast(m)
    assert np.array_equal(got.cpu().numpy(), want)
    for dtype in (torch.uint8, torch.bool):
        back = _decode(got, m.shape, dtype=dtype)
        assert back.dtype == dtype and back.device == DEV and back.shape == m.shape
        assert np.array_equal(back.cpu().numpy().astype(np.uint8), m)


@pytest.mark.parametrize("shape", RC.ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_and_patterns(shape):
    for pattern in RC.PATTERNS:
        m = RC.make_mask(pattern, shape, 21)
        got = _encode(torch.from_numpy(m).to(DEV))
        _check(m, got)
        n = shape[0] * shape[1]
        if pattern == "zeros":
            assert got.numel() == 0
        if pattern == "ones":
            assert got.tolist() == [1, n]
        if pattern == "checker" and shape[0] % 2:               # an odd H alternates across the column wrap too: every set pixel is a run
            assert got.numel() == 2 * (n // 2)
        via_name = R.rle_encode(torch.from_numpy(m).to(DEV))     # the drop-in name on a 2-D CUDA tensor
        assert via_name.device == DEV and torch.equal(via_name, got)


def test_golden_cases():
    z, cases = RC.load_golden()
    for case in cases:
        if not case["two_valued"]:
            continue
        m = RC.case_mask(case)
        got = _encode(torch.from_numpy(m).to(DEV))
        assert np.array_equal(got.cpu().numpy(), z[case["name"] + "/rle"]), case["name"]
        assert R.rle_to_string(got) == case["string"]
        back = _decode(case["string"], m.shape, device=DEV)
        assert np.array_equal(back.cpu().numpy(), m), case["name"]


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.int16, torch.int32, torch.int64], ids=str)
def test_dtypes_alignment_and_views(dtype):
    for shape in [(37, 53), (33, 256), (129, 260)]:              # W % 4 != 0 and == 0
        lm = RC.make_mask("labels6", shape, 31)
        m = (lm != 0).astype(np.uint8)
        t = torch.from_numpy(lm).to(DEV).to(dtype)
        _check(m, _encode(t))
        # the same mask at a base address that is odd in elements: a contiguous [H, W] view of buf[1:]
        buf = torch.zeros(shape[0] * shape[1] + 1, dtype=dtype, device=DEV)
        view = buf[1:].view(shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % (4 * view.element_size()) != 0
        assert torch.equal(_encode(view), _encode(t))
        # a non-contiguous view is made contiguous first
        tt = t.t()
        assert not tt.is_contiguous()
        _check(np.ascontiguousarray(m.T), _encode(tt))
    if dtype == torch.uint8:
        m = RC.make_mask("blobs", (129, 260), 32)
        _check(m, _encode(torch.from_numpy(m * 255).to(DEV)))   # 0 and 255


def test_labels():
    shape = (131, 257)
    lm = RC.make_mask("labels6", shape, 41)
    for dtype in (torch.uint8, torch.int16, torch.int64):
        t = torch.from_numpy(lm).to(DEV).to(dtype)
        labels = [3, 0, 9, 3, -1, 300, 5]                        # repeated, label 0, labels that do not occur (or do not fit the dtype)
        got = _encode(t, labels=labels)
        assert isinstance(got, list) and len(got) == len(labels)
        for c, g in zip(labels, got):
            assert g.dtype == torch.int64 and g.device == DEV
            assert np.array_equal(g.cpu().numpy(), RC.restate_fast(lm == c)), (dtype, c)
        assert got[2].numel() == 0 and got[4].numel() == 0 and got[5].numel() == 0
        assert torch.equal(got[0], got[3])
        base = got[0].untyped_storage().data_ptr()
        assert all(g.untyped_storage().data_ptr() == base for g in got), "the encodings are views of one allocation"
    many = list(range(-2, 20))                                   # more labels than one launch carries
    got = _encode(torch.from_numpy(lm).to(DEV), labels=many)
    for c, g in zip(many, got):
        assert np.array_equal(g.cpu().numpy(), RC.restate_fast(lm == c)), c


def test_stacks():
    shape = (67, 130)
    stack = np.stack([RC.make_mask("labels6", shape, s) for s in (51, 52, 53)])
    stack[1] = 0                                                 # a slice without foreground between two with
    t = torch.from_numpy(stack).to(DEV)
    per_slice = _encode(t)
    nested = _encode(t, labels=range(6))
    assert isinstance(per_slice, list) and len(per_slice) == 3 and len(nested) == 3
    for b in range(3):
        assert torch.equal(per_slice[b], _encode(t[b]))
        assert np.array_equal(per_slice[b].cpu().numpy(), RC.restate_fast(stack[b] != 0))
        own = _encode(t[b], labels=range(6))
        assert len(nested[b]) == 6
        for c in range(6):
            assert torch.equal(nested[b][c], own[c])
            assert np.array_equal(nested[b][c].cpu().numpy(), RC.restate_fast(stack[b] == c))
    assert per_slice[1].numel() == 0
    with pytest.raises(ValueError):
        R.rle_encode(t)                                          # the drop-in name refuses a CUDA stack
    with pytest.raises(NotImplementedError):
        R.rle_encode_device(t.float())


@pytest.mark.parametrize("pattern", ["sparse", "dense"])
def test_scan_levels(pattern):
    """H = 1: every column is a segment, so W counts are scanned.  W > 2048 * 2048: the tiles of 2048 counts need two levels of sums, the
    lower one with more than one workgroup (2100 tiles -> 2 tiles -> 1 workgroup)."""
    W = 2048 * 2048 + 2048 * 51 + 77
    rng = np.random.default_rng(61)
    if pattern == "sparse":
        m = np.zeros((1, W), np.uint8)
        m[0, rng.integers(0, W, 3000)] = 1
        m[0, -1] = 1
        m[0, 2048 * 2048 - 1:2048 * 2048 + 3] = 1
    else:
        m = (rng.random((1, W)) < 0.5).astype(np.uint8)
    got = _encode(torch.from_numpy(m).to(DEV))
    assert np.array_equal(got.cpu().numpy(), RC.restate_fast(m))
    back = _decode(got, m.shape)
    assert np.array_equal(back.cpu().numpy(), m)


def test_decode_inputs_and_errors():
    z, _ = RC.load_golden()
    ov = json.loads(str(z["__overlap__"]))
    shape = tuple(ov["shape"])
    want = np.unpackbits(z["overlap/decoded_bits"])[:shape[0] * shape[1]].reshape(shape)
    on_device = torch.tensor(ov["runs"], device=DEV)
    for runs, kw in ((ov["string"], dict(device=DEV)), (ov["runs"], dict(device="cuda")), (np.asarray(ov["runs"]), dict(device=DEV)),
                     (on_device, {}), (on_device.to(torch.int32), {}), (torch.tensor(ov["runs"]), dict(device=DEV))):
        for dtype in (torch.uint8, torch.bool):
            got = _decode(runs, shape, dtype=dtype, **kw)
            assert got.dtype == dtype and got.device == DEV and np.array_equal(got.cpu().numpy().astype(np.uint8), want)
    via = R.rle_decode(ov["string"], shape, np.uint8, device=DEV)     # the drop-in name with a device requested
    assert via.device == DEV and np.array_equal(via.cpu().numpy(), want)
    # long vertical runs, overlapping and out of order, in a mask of several tiles: columns 3 .. 5 whole, and pieces
    H, W = 300, 77
    runs = [3 * H + 1, 3 * H, 40 * H + 17, 2 * H, 4 * H + 5, 100, 1, 1, 76 * H + 299, 2, 41 * H, 50]
    got = _decode(torch.tensor(runs, device=DEV), (H, W))
    assert np.array_equal(got.cpu().numpy(), RC.decode_restate(runs, (H, W)))
    assert _decode("", (5, 3), device=DEV).sum().item() == 0
    for bad in ([1, 2, 3], [0, 2], [1, -1], [15, 2], "7 10"):
        with pytest.raises(ValueError):
            R.rle_decode_device(bad, (5, 3), device=DEV)
    with pytest.raises(ValueError):
        R.rle_decode_device(on_device[:3], shape)                # an odd count is known without reading the runs
    with pytest.raises(NotImplementedError):
        R.rle_decode_device(on_device, shape, dtype=torch.int32)


def test_decode_long_runs_across_the_chunk_stride():
    """The fill kernel hands the 16384-byte chunks of a long run round robin to gridDim.y = Z waves: one run longer than 2 * Z * 16384
    bytes with Z = 64 (a single run block), and Z = 1 (more than 1024 run blocks) with a run longer than 16384 bytes among short ones."""
    H, W = 1500, 1500
    runs = [7, 2 * 64 * 16384 + 100001, 2200000, 5]                                # (ends off any 16-byte boundary; a short run behind it)
    got = _decode(torch.tensor(runs, device=DEV), (H, W))
    assert np.array_equal(got.cpu().numpy(), RC.decode_restate(runs, (H, W)))
    H, W = 1200, 1200
    m = RC.make_mask("noise", (H, W), 81)
    flat = np.ascontiguousarray(m.T).reshape(-1)
    flat[300003:300003 + 40001] = 1                                                 # one run of 40 k pixels in the noise
    m = np.ascontiguousarray(flat.reshape(W, H).T)
    pairs = RC.restate_fast(m).reshape(-1, 2)
    assert pairs.shape[0] > 1024 * 256 and pairs[:, 1].max() > 16384
    shuffled = pairs[np.random.default_rng(82).permutation(pairs.shape[0])].reshape(-1)
    got = _decode(torch.from_numpy(shuffled).to(DEV), (H, W))
    assert np.array_equal(got.cpu().numpy(), m)


def test_pipeline_merge_crop_argmax_into_rle():
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer, TileMerger

    C, tile, step = 4, 64, 32
    slicer = ImageSlicer((150, 203, 3), tile, step, weight="pyramid")
    g = torch.Generator().manual_seed(71)
    outputs = torch.randn((len(slicer.crops), C, tile, tile), generator=g)
    outputs = torch.nn.functional.avg_pool2d(outputs, 9, stride=1, padding=4)    # smooth logits: regions instead of specks
    merger = TileMerger(slicer.target_shape, C, slicer.weight, device=DEV)
    merger.integrate_batch(outputs.to(DEV), slicer.crops)
    labels_map = merger.merge_crop(slicer, argmax=True, dtype=torch.uint8)
    assert labels_map.shape == (150, 203) and labels_map.dtype == torch.uint8 and labels_map.device == DEV
    got = _encode(labels_map, labels=range(C))
    host = labels_map.cpu().numpy()
    assert len(np.unique(host)) > 1
    for c in range(C):
        assert np.array_equal(got[c].cpu().numpy(), R.rle_encode((host == c).astype(np.uint8))), c
        assert np.array_equal(_decode(got[c], host.shape).cpu().numpy(), (host == c).astype(np.uint8))
