"""The gather kernels of the deferred slab merge (ptb_volume_bands.hip) use no scratch memory and no LDS, and exist as exactly one
instance per source type x (plain tiles | mirror TTA with a linear | a non-linear reduction) x (4-run | scalar) lane shape x result
kind; moving the shared device code into headers left the instance counts of ptb_merge_crop.hip as they were.  Read from the compiler's
resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_volume_bands.hip.txt")


def test_gather_kernels_have_no_scratch(report):
    hits = _find(report, "volume_gather_kernel")
    assert len(hits) == 3 * 3 * 2 * 6      # source dtype x mode x lane shape x PTB_CROP_* kind
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] == 0, (k, r)
        assert r["Occupancy"] >= 3, (k, r)     # (the 8 tile runs + 8 weight runs a lane keeps in flight: <= 168 VGPRs)
    assert len(report) == len(hits)         # nothing else is launched from this translation unit


def test_merge_crop_instances_did_not_move(forced_build):
    report = _report(Path(forced_build["remarks_dir"]) / "ptb_merge_crop.hip.txt")
    assert len(_find(report, "crop_planar_kernel")) == 6            # one per PTB_CROP_* kind
    assert len(_find(report, "crop_last_kernel")) == 4 * 4          # the four non-argmax kinds x CT in {0, 2, 3, 4}
