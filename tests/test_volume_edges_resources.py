"""The 3-D loop-edge kernels (ptb_volume_edges.hip) use no scratch memory: the split kernel keeps its by-value launch descriptor
(tile origins, per-channel affine) in kernel arguments, indexed only by workgroup-uniform values -- run-time indexing that copies
such a struct to scratch once cost the band kernel 18 %.  Read from the compiler's resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_volume_edges.hip.txt")


def test_volume_split_kernels_have_no_scratch(report):
    hits = _find(report, "volume_split_kernel")
    assert len(hits) == 6 * 3 * 2          # input dtype x output dtype x (16-byte / scalar stores)
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] <= 20 * 1024, (k, r)


def test_volume_merge_crop_kernels_have_no_scratch(report):
    hits = {**_find(report, "volume_crop_planar_kernel"), **_find(report, "volume_crop_dhwc_kernel")}
    assert len(hits) >= 6
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
