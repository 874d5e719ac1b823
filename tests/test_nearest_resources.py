"""The feature-transform kernels (ptb_nearest.hip) use no scratch memory, spill nothing and hold no LDS, as DESIGN.md ("Nearest site and
label expansion") states: they are the distance kernels with a second map, the envelope's stack still in the WORKSPACE.  The line passes
stay at eight waves per SIMD -- other waves are all that hides their dependent loads, the feature gather included.  Read from the
compiler's resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report

KERNELS = ("ft_row_kernel", "ft_line_kernel", "ft_gather_kernel")
ELEMENT = {"h": 1, "s": 2, "i": 4, "x": 8}          # the mangled element types of the label maps


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_nearest.hip.txt")


def test_no_scratch_no_spills_no_lds(report):
    assert report
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] == 0, (k, r)


def test_registers_leave_eight_waves_per_simd(report):
    for k, r in report.items():
        assert r["VGPRs"] <= 64 and r["Occupancy"] >= 8, (k, r)
    for k, r in _find(report, "ft_line_kernel").items():
        assert r["VGPRs"] <= 40, (k, r)             # (the int32 instance takes 18, the double-evaluating float32 one 32: as edt_line_kernel)


def test_kernel_instances(report):
    assert len(_find(report, "ft_row_kernel")) == 4 * 2 * 2            # element size x (wide loads | peeled) x (int32 | float32 with spacing)
    for t in ELEMENT:
        for wide in "01":
            for flt in "01":
                assert len(_find(report, f"ft_row_kernelI{t}Lb{wide}ELb{flt}EE")) == 1
    assert len(_find(report, "ft_line_kernel")) == 2                   # int32 | float32 (the last pass is no instance of its own)
    for flt in "01":
        assert len(_find(report, f"ft_line_kernelILb{flt}EE")) == 1
    assert len(_find(report, "ft_gather_kernel")) == 4 * 2             # element size x (wide | peeled)
    for t in ELEMENT:
        for wide in "01":
            assert len(_find(report, f"ft_gather_kernelI{t}Lb{wide}EE")) == 1


def test_no_other_kernel_in_the_translation_unit(report):
    assert all(any(n in k for n in KERNELS) for k in report), sorted(report)
    assert all(any(n in k for k in report) for n in KERNELS), sorted(report)
