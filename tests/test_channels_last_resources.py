"""The channels-last kernels of ptb_channels_last.hip: exactly one instance per (linear | non-linear reduction) x source dtype x
(vector | element loads) for each of the four kernels -- view codes and the channel count are run-time values, there is no per-group or
per-C instance --, no scratch, no spills, and no LDS at all (a view permutes pixels, and a channels-last pixel is one
contiguous run, so nothing is transposed; the budget the design states is 0 bytes, far inside the 64 KB a workgroup may use).  The
planar kernels next to them keep the instance lists of the parent commit: their device code is not touched.  Read from the compiler's
resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_channels_last.hip.txt")


@pytest.mark.parametrize("kernel", ["cl_reduce_kernel", "cl_accum_kernel", "cl_band_kernel", "cl_plan_kernel"])
def test_channels_last_kernels(report, kernel):
    hits = _find(report, kernel)
    assert len(hits) == 2 * 3 * 2, sorted(hits)
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] == 0, (k, r)
        assert r["LDS Size"] <= 64 * 1024, (k, r)
        assert r["Occupancy"] >= 4, (k, r)          # 256-thread workgroups: at least four of them per CU


def test_no_other_kernels_in_the_translation_unit(report):
    assert len(report) == 4 * 12, sorted(report)


@pytest.mark.parametrize("unit, kernel, count", [
    ("ptb_bandplan.hip.txt", "band_plan_kernel", 156),
    ("ptb_views.hip.txt", "view_accum_kernel", 91 - 3 * 7),
    ("ptb_views.hip.txt", "view_plain_kernel", 81 - 3 * 6),
])
def test_planar_kernels_keep_the_parent_commits_instances(forced_build, unit, kernel, count):
    """Instance counts of the planar kernels as compiled when the channels-last kernels arrived (they read dense batches exactly as before);
    the two view kernels less their linear fp32 instances with temporal loads, which nothing selects any more: 3 chunk heights x 7 view
    groups of view_accum_kernel, 3 x 6 of view_plain_kernel."""
    hits = {k: v for k, v in _report(Path(forced_build["remarks_dir"]) / unit).items() if ("%d%s" % (len(kernel), kernel)) in k}
    assert len(hits) == count
