"""The instance-matching kernels (ptb_instances.hip) use no scratch memory and spill nothing: a lane's four ids, keys and IoUs are arrays
indexed by unrolled constants only, and the thresholds of the by-value argument struct are picked by a chain of selects.  Their LDS is
what DESIGN.md ("Instance matching") states: the pair kernel's three 1024-slot tables -- 64-bit key, count and first position of a pair
(16 KiB), id and count of each side (2 x 8 KiB) --, four counts and four sums of the count kernel, nothing elsewhere.  Read from the
compiler's resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report

KERNELS = ("inst_pair_kernel", "inst_mark_kernel", "inst_rank_kernel", "inst_match_kernel", "inst_count_kernel", "inst_finish_kernel", "scan_reduce_kernel",
           "scan_tile_kernel")
LDS = {"inst_pair_kernel": 32768, "inst_mark_kernel": 0, "inst_rank_kernel": 0, "inst_match_kernel": 0, "inst_count_kernel": 48, "inst_finish_kernel": 0,
       "scan_reduce_kernel": 32, "scan_tile_kernel": 32}


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_instances.hip.txt")


def test_no_scratch_no_spills(report):
    assert report
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["VGPRs"] <= 64 and r["Occupancy"] >= 5, (k, r)       # (5: the 32 KiB of the pair kernel, five workgroups per CU)


def test_lds_is_what_the_design_states(report):
    for name, lds in LDS.items():
        for k, r in _find(report, name).items():
            assert r["LDS Size"] == lds, (k, r)


def test_kernel_instances(report):
    assert len(_find(report, "inst_pair_kernel")) == 2                 # 16-byte loads | element loads
    for wide in "01":
        assert len(_find(report, f"inst_pair_kernelILb{wide}EE")) == 1
    for single in ("inst_mark_kernel", "inst_rank_kernel", "inst_match_kernel", "inst_count_kernel", "inst_finish_kernel"):
        assert len(_find(report, single)) == 1, single
    assert len(_find(report, "scan_reduce_kernel")) == 2 and len(_find(report, "scan_tile_kernel")) == 2     # 32-bit counts, 64-bit sums


def test_no_other_kernel_in_the_translation_unit(report):
    assert all(any(n in k for n in KERNELS) for k in report), sorted(report)
    assert all(any(n in k for k in report) for n in KERNELS), sorted(report)
