"""The distance-map loss kernels (ptb_distance_loss.hip) use no scratch memory and spill nothing in any instance, and hold only the LDS of
their workgroup sums, as DESIGN.md ("Distance-map losses") states.  The occupancy floors are what the compiler reported for the finished
kernels (recorded there as well): eight waves per SIMD everywhere but in the instances that hold 8 or 16 softmax channels of four
positions in registers.  Read from the compiler's resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report

KERNELS = ("dl_mask_kernel", "dl_fwd_kernel", "dl_bwd_kernel", "dl_finish_kernel")
CHANNELS = {"4": "Li4E", "8": "Li8E", "16": "Li16E", "sweep": "Li0E", "independent": "Lin1E"}      # the mangled CR of an instance
# waves per SIMD, as reported: [kernel][kind][CR]; the Hausdorff form reads a second map and carries the target
FLOOR = {
    "dl_mask_kernel": {None: {"4": 8, "8": 8, "16": 5, "sweep": 8, "independent": 8}},
    "dl_fwd_kernel": {0: {"4": 8, "8": 8, "16": 4, "sweep": 8, "independent": 8}, 1: {"4": 8, "8": 7, "16": 3, "sweep": 7, "independent": 8}},
    "dl_bwd_kernel": {0: {"4": 8, "8": 8, "16": 5, "sweep": 8, "independent": 8}, 1: {"4": 8, "8": 6, "16": 4, "sweep": 7, "independent": 8}},
}


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_distance_loss.hip.txt")


def _instances(report, kernel, kind, cr):
    prefix = f"{kernel}I" + (f"Li{kind}E" if kind is not None else "") + CHANNELS[cr] + "Lb"
    return _find(report, prefix)


def test_no_scratch_no_spills(report):
    assert report
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)


def test_lds_is_the_workgroup_sums(report):
    for k, r in report.items():
        want = 64 if "dl_fwd_kernel" in k else 4096 if "dl_finish_kernel" in k else 0      # 4 waves / 256 lanes x (fp64 sum + int64 count)
        assert r["LDS Size"] == want, (k, r)


def test_occupancy_floors(report):
    for kernel, kinds in FLOOR.items():
        for kind, floors in kinds.items():
            for cr, floor in floors.items():
                hits = _instances(report, kernel, kind, cr)
                assert len(hits) == 2, (kernel, kind, cr, sorted(hits))            # 16-byte accesses | peeled
                for k, r in hits.items():
                    assert r["Occupancy"] >= floor, (k, r)
    for k, r in _find(report, "dl_finish_kernel").items():
        assert r["Occupancy"] >= 8, (k, r)


def test_kernel_instances(report):
    assert len(_find(report, "dl_mask_kernel")) == 5 * 2                       # channel handling x (wide | peeled)
    assert len(_find(report, "dl_fwd_kernel")) == 2 * 5 * 2                    # (boundary | Hausdorff) x channel handling x (wide | peeled)
    assert len(_find(report, "dl_bwd_kernel")) == 2 * 5 * 2
    assert len(_find(report, "dl_finish_kernel")) == 1
    for wide in "01":
        for cr in CHANNELS.values():
            assert len(_find(report, f"dl_mask_kernelI{cr}Lb{wide}EE")) == 1
            for kind in "01":
                assert len(_find(report, f"dl_fwd_kernelILi{kind}E{cr}Lb{wide}EE")) == 1
                assert len(_find(report, f"dl_bwd_kernelILi{kind}E{cr}Lb{wide}EE")) == 1


def test_no_other_kernel_in_the_translation_unit(report):
    assert all(any(n in k for n in KERNELS) for k in report), sorted(report)
    assert all(any(n in k for k in report) for n in KERNELS), sorted(report)
