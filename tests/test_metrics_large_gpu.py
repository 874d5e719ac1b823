"""GPU: a confusion matrix over more than 2^31 positions (every offset of csrc/ptb_confusion.hip is 64-bit).  The maps are zeros with
a few written slices, so the expected matrix is known without a host computation."""
import pytest
import torch

from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import metrics as M

pytestmark = pytest.mark.gpu

BIG = 2 ** 31 + 2 ** 20 + 3


def test_confusion_matrix_beyond_2g_positions():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 6e9:
        pytest.skip(f"needs 6 GB of free device memory for two maps of 2^31 + 2^20 + 3 bytes, {free / 1e9:.1f} GB are free")
    pred = torch.zeros(BIG, dtype=torch.uint8, device=dev)
    target = torch.zeros(BIG, dtype=torch.uint8, device=dev)
    K = 4
    want = torch.zeros((K, K), dtype=torch.int64)
    pieces = [(0, 1000, 1, 2), (2 ** 31 - 7, 2 ** 31 + 9, 2, 2), (2 ** 31 + 4096, 2 ** 31 + 4096 + 123457, 3, 1), (BIG - 5, BIG, 1, 3)]     # [a, b): pred, target
    for a, b, p, t in pieces:
        pred[a:b] = p
        target[a:b] = t
        want[t, p] += b - a
    target[BIG - 1] = 255                                        # the very last position is ignored ...
    want[3, 1] -= 1
    pred[2 ** 31 + 17] = 200                                     # ... and one beyond 2^31 is out of range
    want[0, 0] = BIG - int(want.sum()) - 2
    before = N.calls
    got = M.confusion_matrix(pred, target, K, ignore_index=255)
    assert N.calls == before + 1
    assert torch.equal(got.cpu(), want) and int(got.sum()) == BIG - 2
    with pytest.raises(ValueError, match=r"\b1 position"):
        M.confusion_matrix(pred, target, K, ignore_index=255, strict=True)
