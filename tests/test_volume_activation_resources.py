"""The kernels of ptb_volume_activation.hip: one instance per source dtype x layout x lane width of the reduce and accumulate kernels,
one per source dtype x layout x lane width x result kind of the gather kernel -- activation, temperature, reduction, masks, C and all
extents are run-time values --, no scratch, no spills, no LDS.  Read from the compiler's resource remarks of the session's forced rebuild.
(The sibling tests show that the planar and channels-last units kept their instances.)"""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_volume_activation.hip.txt")


@pytest.mark.parametrize("kernel, count, occupancy", [
    # the 4-voxel dense lanes keep 2 x 8 channels x 4 voxels = 64 floats of channel state (the view in flight and the view sum) next to
    # their addresses and the accumulator run: the 168-register step, three waves per SIMD
    ("act_reduce_kernel", 3 * 2 * 2, 3),
    ("act_accum_kernel", 3 * 2 * 2, 3),
    ("act_gather_kernel", 3 * 2 * 2 * 6, 2),        # ... and 96 floats with the blend accumulator: beyond that step, two waves
])
def test_activation_kernels(report, kernel, count, occupancy):
    hits = _find(report, kernel)
    assert len(hits) == count, sorted(hits)
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] == 0, (k, r)
        assert r["Occupancy"] >= occupancy, (k, r)


def test_no_other_kernels_in_the_translation_unit(report):
    assert len(report) == 12 + 12 + 72, sorted(report)
