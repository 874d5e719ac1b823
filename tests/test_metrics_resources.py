"""The confusion-matrix kernels (ptb_confusion.hip) use no scratch memory and spill nothing: a lane's run of positions, its running
best per position and its one open (key, length) pair are arrays indexed by unrolled constants only.  Their LDS is the dynamic
histogram alone -- no static LDS in front of it -- whose size ptb_confusion_plan states: at most 64 KiB, far below the
160 KiB of a CU.  Read from the compiler's resource remarks of the session's forced rebuild."""
import ctypes
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report

KERNELS = ("confusion_labels_kernel", "confusion_logits_kernel")


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_confusion.hip.txt")


def test_no_scratch_no_spills_no_static_lds(report):
    assert report
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] == 0, (k, r)                  # the histogram is the launch's dynamic LDS: ptb_confusion_plan
        assert r["VGPRs"] <= 128 and r["Occupancy"] >= 4, (k, r)


def test_dynamic_lds_is_what_the_design_states(forced_build):
    lib = ctypes.CDLL(str(Path(forced_build["lib_dir"]) / "libptb_hip.so"))
    worst = 0
    for K in range(1, 257):
        rb, lds = ctypes.c_int(), ctypes.c_int()
        assert lib.ptb_confusion_plan(K, ctypes.byref(rb), ctypes.byref(lds)) == 0
        rows = min(K, 16384 // K)
        assert lds.value == rows * K * 4 and rb.value * rows >= K > (rb.value - 1) * rows
        worst = max(worst, lds.value)
    assert worst == 64 * 1024 < 160 * 1024


def test_kernel_instances(report):
    assert len(_find(report, "confusion_labels_kernel")) == 4 * 4         # pred element size x target element size
    assert len(_find(report, "confusion_logits_kernel")) == 3 * 4         # fp32 | fp16 | bf16 x target element size
    hot = _find(report, "confusion_labels_kernelIhhEE").popitem()[1]       # the uint8 pair of merge_crop(argmax=True, dtype=torch.uint8)
    assert hot["VGPRs"] <= 64, hot


def test_no_other_kernel_in_the_translation_unit(report):
    assert all(any(n in k for n in KERNELS) for k in report), sorted(report)
    assert all(any(n in k for k in report) for n in KERNELS), sorted(report)
