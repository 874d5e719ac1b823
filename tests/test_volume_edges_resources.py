"""The 3-D loop-edge kernels (ptb_volume_edges.hip) and the merge + crop kernels (ptb_merge_crop.hip) use no scratch memory: the
split kernel keeps its by-value launch descriptor (tile origins, per-channel affine) in kernel arguments, indexed only by
workgroup-uniform values -- run-time indexing that copies such a struct to scratch once cost the band kernel 18 %.  Read from the
compiler's resource remarks of the session's forced rebuild."""
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


def test_merge_crop_kernels_have_no_scratch(forced_build):
    """The merge + crop kernels shared by ptb_merge_crop and ptb_volume_merge_crop (ptb_merge_crop.hip): no scratch, and LDS only in
    the fp32 channel-last instances, which exchange their stores through it."""
    report = _report(Path(forced_build["remarks_dir"]) / "ptb_merge_crop.hip.txt")
    planar, last = _find(report, "crop_planar_kernel"), _find(report, "crop_last_kernel")
    assert len(planar) == 6                # PTB_CROP_* kinds
    assert len(last) == 4 * 4              # non-argmax kinds x (2, 3, 4 channels in registers | any C)
    repack = {k for k in last if any(f"crop_last_kernelILi0ELi{ct}EE" in k for ct in (2, 3, 4))}
    assert len(repack) == 3
    for k, r in {**planar, **last}.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        if k in repack:
            assert 0 < r["LDS Size"] <= 16 * 1024, (k, r)
        else:
            assert r["LDS Size"] == 0, (k, r)
