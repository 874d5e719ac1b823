"""The 3-D resampling kernel (ptb_volume_resample.hip) uses no scratch memory and at most 40 KB of LDS: a lane's taps are arrays indexed
by unrolled constants only, and the LDS brick is sized so that at least four workgroups share a CU's 160 KB.  Read from the compiler's
resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_volume_resample.hip.txt")


def test_volume_resize_kernels(report):
    hits = _find(report, "volume_resize_kernel")
    assert len(hits) == 6 * 3 * 2          # input dtype x output dtype x (LDS-staged | direct gathers)
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] <= 40 * 1024, (k, r)
        assert r["LDS Size"] == (2560 * 4 if "Lb1EEE" in k else 0), (k, r)       # STAGE: the brick; direct gathers: none
        if "Lb1EEE" in k:
            assert r["VGPRs"] <= 64 and r["Occupancy"] >= 8, (k, r)


def test_no_other_kernel_in_the_translation_unit(report):
    assert all("volume_resize_kernel" in k for k in report), sorted(report)
