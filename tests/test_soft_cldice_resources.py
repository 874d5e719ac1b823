"""The soft-skeleton kernels (ptb_softskel.hip) use no scratch memory and spill nothing, and hold the LDS planes DESIGN.md ("Soft clDice")
states with the register figures pinned here.  Read from the compiler's resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report

KERNELS = ("ss_fwd_kernel", "ss_finish_kernel", "ss_bwd_kernel", "ss_act_bwd_kernel")


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_softskel.hip.txt")


def test_no_scratch_no_spills(report):
    assert report
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (k, r)


def test_lds_plans(report):
    for R, skeleton_only in ((5, True), (5, False), (10, True), (10, False)):                  # two planes of (32 + 2 R + 2)^2 floats; the loss: and 4 x 4 doubles
        (r,) = _find(report, f"ss_fwd_kernelILi{R}ELb{0 if skeleton_only else 1}EE").values()
        assert r["LDS Size"] == 2 * 4 * (32 + 2 * R + 2) ** 2 + (0 if skeleton_only else 128), r
    for T, R in ((32, 5), (24, 7), (16, 10)):                                                  # three planes of the tile + 2 R, go, gv and the selection bytes on the tile + R
        (r,) = _find(report, f"ss_bwd_kernelINS_5SsBwdILi{T}ELi{R}EEEE").values()
        assert r["LDS Size"] == 3 * 4 * (T + 4 * R + 2) ** 2 + 9 * (T + 2 * R + 2) ** 2 <= 160 * 1024 // 3, r
        assert r["VGPRs"] <= 168 and r["Occupancy"] >= 3, r                                    # three workgroups a CU by LDS: 3 waves a SIMD (160 / 150 / 140 reported)
    (r,) = _find(report, "ss_finish_kernel").values()
    assert r["LDS Size"] == 4 * 8 * 256, r
    (r,) = _find(report, "ss_act_bwd_kernel").values()
    assert r["LDS Size"] == 0, r


def test_registers_of_the_forward(report):
    for k, r in _find(report, "ss_fwd_kernel").items():
        assert r["VGPRs"] <= 64 and r["Occupancy"] >= 6, (k, r)                                # (26 / 40 reported; the R = 10 instances are LDS-bound at 7 / 6)


def test_no_other_kernel_in_the_translation_unit(report):
    assert len(report) == 4 + 1 + 3 + 1
    assert all(any(n in k for n in KERNELS) for k in report), sorted(report)
