"""The hard-example-mining kernels (ptb_hard_mining.hip) use no scratch memory and spill nothing in any instance, and hold only the LDS
that DESIGN.md ("Hard-example mining") states: the 256-bin histogram (and the two workgroup counts of the loss pass), the scan of the
pick, the workgroup sums.  The occupancy floors are what the compiler reported for the finished kernels (recorded there as well): eight
waves per SIMD everywhere but in the instances that hold 16 softmax channels of four positions in registers.  Read from the compiler's
resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report

KERNELS = ("hm_loss_kernel", "hm_hist_kernel", "hm_pick_kernel", "hm_sum_kernel", "hm_finish_kernel", "hm_bwd_kernel")
CHANNELS = {"4": "Li4E", "8": "Li8E", "16": "Li16E", "sweep": "Li0E", "independent": "Lin1E"}      # the mangled CR of an instance
# waves per SIMD, as reported: [kernel][CR]
FLOOR = {
    "hm_loss_kernel": {"4": 8, "8": 8, "16": 6, "sweep": 8, "independent": 8},
    "hm_bwd_kernel": {"4": 8, "8": 8, "16": 4, "sweep": 8, "independent": 8},
}
# bytes per workgroup: 256 bins (+ the counts n and above-t0) | 256 bins | the scan | 4 waves x (fp64 sum + two counts) | 256 lanes x the same
LDS = {"hm_loss_kernel": 256 * 4 + 8, "hm_hist_kernel": 256 * 4, "hm_pick_kernel": 256 * 4, "hm_sum_kernel": 4 * 16, "hm_finish_kernel": 256 * 16,
       "hm_bwd_kernel": 0}


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_hard_mining.hip.txt")


def test_no_scratch_no_spills(report):
    assert report
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)


def test_lds_is_the_histograms_and_the_workgroup_sums(report):
    for k, r in report.items():
        (kernel,) = [n for n in KERNELS if n in k]
        assert r["LDS Size"] == LDS[kernel], (k, r)


def test_occupancy_floors(report):
    for kernel, floors in FLOOR.items():
        for cr, floor in floors.items():
            hits = _find(report, f"{kernel}I{CHANNELS[cr]}Lb")
            assert len(hits) == 2, (kernel, cr, sorted(hits))                   # 16-byte accesses | peeled
            for k, r in hits.items():
                assert r["Occupancy"] >= floor, (k, r)
    for kernel in ("hm_hist_kernel", "hm_pick_kernel", "hm_sum_kernel", "hm_finish_kernel"):
        for k, r in _find(report, kernel).items():
            assert r["Occupancy"] >= 8, (k, r)


def test_kernel_instances(report):
    assert len(_find(report, "hm_loss_kernel")) == 5 * 2                       # channel handling x (wide | peeled)
    assert len(_find(report, "hm_bwd_kernel")) == 5 * 2
    assert len(_find(report, "hm_hist_kernel")) == 2                           # wide | peeled map
    assert len(_find(report, "hm_sum_kernel")) == 2
    assert len(_find(report, "hm_pick_kernel")) == 1 and len(_find(report, "hm_finish_kernel")) == 1
    for wide in "01":
        for cr in CHANNELS.values():
            assert len(_find(report, f"hm_loss_kernelI{cr}Lb{wide}EE")) == 1
            assert len(_find(report, f"hm_bwd_kernelI{cr}Lb{wide}EE")) == 1
        assert len(_find(report, f"hm_hist_kernelILb{wide}EE")) == 1 and len(_find(report, f"hm_sum_kernelILb{wide}EE")) == 1


def test_no_other_kernel_in_the_translation_unit(report):
    assert all(any(n in k for n in KERNELS) for k in report), sorted(report)
    assert all(any(n in k for k in report) for n in KERNELS), sorted(report)
