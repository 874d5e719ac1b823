"""The channels_last_3d kernels of ptb_volume_channels_last.hip: exactly one instance per source dtype x (linear | non-linear
reduction) x (vector | element loads) of the reduce and accumulate kernels, one per source dtype x mode x (vector | element loads) x
result kind of the gather kernel -- C, masks, reduction, extents and result layout are run-time values --, no scratch, no spills, no LDS.
The planar units next to them keep their instance counts: the launch arguments moved into a header, their device code did not change.
Read from the compiler's resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_volume_channels_last.hip.txt")


@pytest.mark.parametrize("kernel, count, occupancy", [
    ("cl3_reduce_kernel", 3 * 2 * 2, 4),            # 256-thread workgroups: at least four of them per CU, like the 2-D channels-last kernels
    ("cl3_accum_kernel", 3 * 2 * 2, 4),
    ("cl3_gather_kernel", 3 * 3 * 2 * 6, 3),        # the bound of the planar gather (a lane here keeps fewer loads in flight)
])
def test_channels_last_3d_kernels(report, kernel, count, occupancy):
    hits = _find(report, kernel)
    assert len(hits) == count, sorted(hits)
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] == 0, (k, r)
        assert r["Occupancy"] >= occupancy, (k, r)


def test_no_other_kernels_in_the_translation_unit(report):
    assert len(report) == 12 + 12 + 108, sorted(report)


@pytest.mark.parametrize("unit, kernel, count", [
    ("ptb_volume_bands.hip.txt", "volume_gather_kernel", 3 * 3 * 2 * 6),
    ("ptb_volume_tta.hip.txt", "volume_mirror_kernel", 2 * 2),
    ("ptb_volume_tta.hip.txt", "volume_mirror_reduce_kernel", 3 * 2 * 2),
    ("ptb_volume_tta.hip.txt", "volume_mirror_accumulate_kernel", 3 * 2 * 2),
    ("ptb_merge_crop.hip.txt", "crop_planar_kernel", 6),
    ("ptb_merge_crop.hip.txt", "crop_last_kernel", 4 * 4),
])
def test_planar_units_keep_their_instances(forced_build, unit, kernel, count):
    report = _report(Path(forced_build["remarks_dir"]) / unit)
    assert len(_find(report, kernel)) == count
    if unit != "ptb_merge_crop.hip.txt":
        assert len(report) == (108 if "bands" in unit else 4 + 12 + 12)      # nothing else is launched from these units
