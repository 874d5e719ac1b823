"""CPU: the restatement of tests/metrics_cases.py against hand-written matrices, the CPU-tensor path of utils.metrics against the
restatement over the shared case list, the error table, ``out=`` accumulation, ``strict`` and ``segmentation_scores``."""
import math

import numpy as np
import pytest
import torch

import metrics_cases as MC
from pytorch_toolbelt_amd import utils as U
from pytorch_toolbelt_amd.utils import metrics as M


def test_exported_like_rle():
    assert U.confusion_matrix is M.confusion_matrix and U.segmentation_scores is M.segmentation_scores
    assert U.confusion_matrix_from_logits is M.confusion_matrix_from_logits
    assert "no counterpart" in M.__doc__


def test_restatement_on_hand_written_matrices():
    pred, target = [0, 1, 1, 2, 2, 2, 0], [0, 1, 2, 2, 2, 0, 0]
    want = np.array([[2, 0, 1], [0, 1, 0], [0, 1, 2]])
    for fn in (MC.restate_loop, MC.restate):
        cm, invalid = fn(np.array(pred), np.array(target), 3)
        assert np.array_equal(cm, want) and invalid == 0
    # ignore_index inside [0, K): the target-0 row empties; an ignored position may hold any pred
    for fn in (MC.restate_loop, MC.restate):
        cm, invalid = fn(np.array(pred + [77]), np.array(target + [0]), 3, ignore_index=0)
        assert np.array_equal(cm, [[0, 0, 0], [0, 1, 0], [0, 1, 2]]) and invalid == 0
    # out of range on either side is skipped and counted; an ignored target is not
    p, t = np.array([0, 5, 1, -1, 1, 0]), np.array([0, 0, 9, 1, -100, 255])
    for fn in (MC.restate_loop, MC.restate):
        cm, invalid = fn(p, t, 2, ignore_index=-100)
        assert np.array_equal(cm, [[1, 0], [0, 0]]) and invalid == 4
    x = np.array([[[1.0, 2.0, np.nan, np.nan, -0.0, -np.inf, np.inf]], [[1.0, 1.0, 0.0, np.nan, 0.0, -np.inf, np.inf]], [[0.0, 3.0, 5.0, 1.0, 0.0, 0.0, np.inf]]])
    assert MC.restate_argmax(x.transpose(1, 0, 2)).tolist() == [[0, 2, 0, 0, 0, 2, 0]]
    assert MC.restate_argmax(np.array([[[0.5, 0.25, np.nan, 0.26]]]), 0.25).tolist() == [[1, 0, 0, 1]]


def test_bincount_restatement_equals_the_loop():
    for case in MC.label_cases():
        if case[1] > 2 * MC.CHUNK + 17:
            continue
        p, t = MC.build_case(case)
        a, b = MC.restate_loop(p, t, case[2], case[6]), MC.restate(p, t, case[2], case[6])
        assert np.array_equal(a[0], b[0]) and a[1] == b[1], case[0]


@pytest.mark.parametrize("case", MC.label_cases(), ids=lambda c: c[0])
def test_cpu_path_over_the_case_list(case):
    name, n, K, pd, td, content, ignore, hostile = case
    p, t = MC.build_case(case)
    want, invalid = MC.restate(p, t, K, ignore)
    got = M.confusion_matrix(torch.from_numpy(p), torch.from_numpy(t), K, ignore_index=ignore)
    assert got.dtype == torch.int64 and got.shape == (K, K) and np.array_equal(got.numpy(), want)
    assert int(want.sum()) + invalid <= n and (not hostile or n == 0 or invalid > 0)
    if invalid:
        with pytest.raises(ValueError, match=str(invalid)):
            M.confusion_matrix(torch.from_numpy(p), torch.from_numpy(t), K, ignore_index=ignore, strict=True)
    else:
        assert torch.equal(M.confusion_matrix(torch.from_numpy(p), torch.from_numpy(t), K, ignore_index=ignore, strict=True), got)


def test_per_sample_and_out():
    p, t = MC.make_pair("blobs", 3 * 1001, 5, 7)
    p, t = torch.from_numpy(p).view(3, 7, 143), torch.from_numpy(t).view(3, 7, 143)
    per = M.confusion_matrix(p, t, 5, per_sample=True)
    assert per.shape == (3, 5, 5)
    for b in range(3):
        assert torch.equal(per[b], M.confusion_matrix(p[b], t[b], 5))
    pooled = M.confusion_matrix(p, t, 5)
    assert torch.equal(per.sum(0), pooled) and np.array_equal(per.numpy(), MC.restate(p.numpy(), t.numpy(), 5, per_sample=True)[0])
    out = torch.full((5, 5), 2 ** 32 - 3, dtype=torch.int64)
    back = M.confusion_matrix(p, t, 5, out=out)
    assert back is out and torch.equal(out, pooled + (2 ** 32 - 3))
    M.confusion_matrix(p, t, 5, out=out)
    assert torch.equal(out, 2 * pooled + (2 ** 32 - 3))
    # empty inputs: zeros, or out unchanged
    e = torch.zeros((0, 4), dtype=torch.uint8)
    assert torch.equal(M.confusion_matrix(e, e, 3), torch.zeros((3, 3), dtype=torch.int64))
    assert M.confusion_matrix(e, e, 3, per_sample=True).shape == (0, 3, 3)
    assert torch.equal(M.confusion_matrix(e, e, 5, out=out), 2 * pooled + (2 ** 32 - 3))
    # a non-contiguous view counts like its contiguous copy
    assert torch.equal(M.confusion_matrix(p.transpose(1, 2), t.transpose(1, 2), 5), pooled)


def test_errors():
    u = torch.zeros(8, dtype=torch.uint8)
    with pytest.raises(TypeError):
        M.confusion_matrix(np.zeros(8, np.uint8), u, 2)
    with pytest.raises(TypeError):
        M.confusion_matrix(u.float(), u, 2)
    with pytest.raises(TypeError):
        M.confusion_matrix(u, u.double(), 2)
    with pytest.raises(ValueError):
        M.confusion_matrix(u, u[:7], 2)
    with pytest.raises(ValueError):
        M.confusion_matrix(u, u, 0)
    with pytest.raises(ValueError):
        M.confusion_matrix(u, u, 2, per_sample=True)                       # 1-d: no sample dimension
    with pytest.raises(ValueError):
        M.confusion_matrix(u[0], u[0], 2, per_sample=True)                 # 0-d
    for bad in (torch.zeros((2, 3), dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int32), torch.zeros((1, 2, 2), dtype=torch.int64)):
        with pytest.raises(ValueError):
            M.confusion_matrix(u, u, 2, out=bad)
    with pytest.raises(ValueError):
        M.confusion_matrix(u, u, 2, ignore_index=1 << 63)
    lg = torch.zeros((2, 3, 4, 5))
    tg = torch.zeros((2, 4, 5), dtype=torch.int64)
    with pytest.raises(TypeError):
        M.confusion_matrix_from_logits(lg.double(), tg)
    with pytest.raises(TypeError):
        M.confusion_matrix_from_logits(lg, tg.float())
    with pytest.raises(ValueError):
        M.confusion_matrix_from_logits(lg, tg[:, :3])
    with pytest.raises(ValueError):
        M.confusion_matrix_from_logits(lg, tg, out=torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(TypeError):
        M.segmentation_scores([[1, 0], [0, 1]])
    with pytest.raises(ValueError):
        M.segmentation_scores(torch.zeros((2, 3)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=str)
def test_logits_cpu_path(dtype):
    rng = np.random.default_rng(5)
    for shape in [(2, 1, 5, 13), (2, 2, 5, 13), (1, 4, 3, 7, 11), (2, 19, 9, 9)]:
        x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dtype)
        x.view(-1)[::7] = 0.5                                               # ties
        x.view(-1)[::31] = float("nan")
        t = torch.from_numpy(rng.integers(0, max(shape[1], 2), (shape[0],) + shape[2:]))
        K = max(shape[1], 2)
        pred = MC.restate_argmax(x.float().numpy(), 0.25)
        want, _ = MC.restate(pred, t.numpy(), K)
        got = M.confusion_matrix_from_logits(x, t, threshold=0.25)
        assert np.array_equal(got.numpy(), want), shape
        assert torch.equal(got, M.confusion_matrix(torch.from_numpy(pred), t, K))
        per = M.confusion_matrix_from_logits(x, t, threshold=0.25, per_sample=True)
        assert per.shape == (shape[0], K, K) and torch.equal(per.sum(0), got)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_segmentation_scores():
    cm = torch.tensor([[50, 2, 0, 3], [4, 30, 0, 1], [0, 0, 0, 0], [7, 0, 0, 11]])          # class 2 is absent: NaN everywhere
    got, want = M.segmentation_scores(cm), MC.restate_scores(cm.numpy())
    for k in ("iou", "dice", "precision", "recall"):
        assert got[k].dtype == torch.float64 and got[k].shape == (4,) and _same(got[k].numpy(), want[k]), k
        assert math.isnan(float(got[k][2]))
    assert float(got["iou"][0]) == 50 / 66 and float(got["dice"][3]) == 22 / 33 and float(got["accuracy"]) == 91 / 108
    for k in ("mean_iou", "mean_dice"):
        assert np.allclose(got[k].numpy(), want[k], rtol=1e-12, atol=0) and not math.isnan(float(got[k]))
    assert float(got["accuracy"]) == float(want["accuracy"])
    # an empty matrix: every score is NaN; a batch of matrices scores matrix by matrix
    empty = M.segmentation_scores(torch.zeros((3, 3), dtype=torch.int64))
    assert all(bool(torch.isnan(v).all()) for v in empty.values())
    rng = np.random.default_rng(3)
    stack = torch.from_numpy(rng.integers(0, 10 ** 9, (2, 5, 256, 256)))
    got, want = M.segmentation_scores(stack), MC.restate_scores(stack.numpy())
    for k in ("iou", "dice", "precision", "recall", "accuracy"):
        assert _same(got[k].numpy(), want[k]), k
    for k in ("mean_iou", "mean_dice"):
        assert got[k].shape == (2, 5) and np.allclose(got[k].numpy(), want[k], rtol=1e-12, atol=0)
