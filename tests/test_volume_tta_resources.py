"""The mirror TTA kernels of ptb_volume_tta.hip use no scratch memory and no LDS (flips are index reversals done in registers), with
exactly one instance per element type x reduction kind x (4-run | scalar) lane shape; the split kernel that writes the mirror views
(ptb_volume_edges.hip) has no scratch and stays within the split's LDS budget.  Read from the compiler's resource remarks of the
session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_volume_tta.hip.txt")


@pytest.mark.parametrize("kernel, count", [
    ("volume_mirror_kernel", 2 * 2),                    # element size (4: fp32, 2: fp16 / bf16) x (4-run | scalar)
    ("volume_mirror_reduce_kernel", 3 * 2 * 2),         # source dtype x (linear | non-linear reduction) x (4-run | scalar)
    ("volume_mirror_accumulate_kernel", 3 * 2 * 2),
])
def test_mirror_kernels_have_no_scratch(report, kernel, count):
    hits = _find(report, kernel)
    assert len(hits) == count
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] == 0, (k, r)


def test_split_with_views_keeps_its_lds_budget(forced_build):
    """volume_split_views_kernel (ptb_volume_split_mirror) stages the chunk as volume_split_kernel does: the same instances, no scratch,
    the same LDS budget."""
    report = _report(Path(forced_build["remarks_dir"]) / "ptb_volume_edges.hip.txt")
    plain, views = _find(report, "volume_split_kernel"), _find(report, "volume_split_views_kernel")
    assert len(plain) == len(views) == 6 * 3 * 2          # input dtype x output dtype x (16-byte / scalar stores)
    for k, r in {**plain, **views}.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] <= 20 * 1024, (k, r)
