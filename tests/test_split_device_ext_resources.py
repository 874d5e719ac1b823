"""The 2-D split kernels of ptb_edges.hip (every input x output dtype instance of the LDS-scatter kernel, for each chunk-rows setting, and of
the scalar kernel) use no scratch memory: the launch descriptor -- tile origins, per-channel affine, border -- stays in kernel
arguments, indexed only by workgroup-uniform values.  Read from the compiler's resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_edges.hip.txt")


def test_split_kernels_have_no_scratch(report):
    hits = _find(report, "edge_split_kernel")
    assert len(hits) == 3 * 3 * 3          # chunk rows x input dtype x output dtype
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] <= 16 * 1024, (k, r)


def test_scalar_split_kernels_have_no_scratch(report):
    hits = _find(report, "edge_split_scalar_kernel")
    assert len(hits) == 3 * 3              # input dtype x output dtype
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
