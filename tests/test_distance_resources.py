"""The distance-transform kernels (ptb_distance.hip) use no scratch memory, spill nothing and hold no LDS, as DESIGN.md ("Distance
transform") states: the row pass keeps a lane's four values, indices and results in arrays indexed by unrolled constants only and scans
with wave shuffles; the line passes keep the envelope's stack in the WORKSPACE (laid out [height][line]) with its top entry in
registers -- a private stack array would be scratch.  Both stay far below 64 VGPRs, so eight waves per SIMD fit: the line passes hide
the latency of their dependent loads behind other waves and nothing else.  Read from the compiler's resource remarks of the session's
forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report

KERNELS = ("edt_row_kernel", "edt_line_kernel")
ELEMENT = {"h": 1, "s": 2, "i": 4, "x": 8}          # the mangled element types of the label maps


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_distance.hip.txt")


def test_no_scratch_no_spills_no_lds(report):
    assert report
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] == 0, (k, r)


def test_registers_leave_eight_waves_per_simd(report):
    for k, r in report.items():
        assert r["VGPRs"] <= 64 and r["Occupancy"] >= 8, (k, r)
    for k, r in _find(report, "edt_line_kernel").items():
        assert r["VGPRs"] <= 40, (k, r)             # (the int32 instances take 18, the double-evaluating float32 ones 32)


def test_kernel_instances(report):
    assert len(_find(report, "edt_row_kernel")) == 4 * 2 * 2           # element size x (wide loads | peeled) x (int32 | float32 with spacing)
    for t in ELEMENT:
        for wide in "01":
            for flt in "01":
                assert len(_find(report, f"edt_row_kernelI{t}Lb{wide}ELb{flt}EE")) == 1
    assert len(_find(report, "edt_line_kernel")) == 2 * 2              # (int32 | float32) x (a further axis follows | the last pass)
    for flt in "01":
        for last in "01":
            assert len(_find(report, f"edt_line_kernelILb{flt}ELb{last}EE")) == 1


def test_no_other_kernel_in_the_translation_unit(report):
    assert all(any(n in k for n in KERNELS) for k in report), sorted(report)
    assert all(any(n in k for k in report) for n in KERNELS), sorted(report)
