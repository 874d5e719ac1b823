"""The surface-metric kernels (ptb_surface.hip) use no scratch memory and spill nothing, and hold exactly the LDS that DESIGN.md ("Surface
metrics") states: the border kernel its 32 class counters (128 B), the statistics pass two private 256-bin histograms and a double per wave
(2048 + 32 B), the further histogram passes the two histograms (2048 B), the pick kernel its 256-word scan (1024 B), the upper-statistic
pass and the finishing kernel none.  (A lane's 16 flags are four words indexed by constants only: a run-time index would have made the
compiler move them to LDS, 4 KiB per workgroup, or to scratch.)  All stay within 64 VGPRs, so eight waves per SIMD fit: the sample passes
hide the latency of their gathered loads behind other waves.  Read from the compiler's resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report

LDS = {"surf_border_kernel": 128, "surf_stats_kernel": 2080, "surf_hist_kernel": 2048, "surf_upper_kernel": 0, "surf_pick_kernel": 1024,
       "surf_finish_kernel": 0}
ELEMENT = {"h": 1, "s": 2, "i": 4, "x": 8}          # the mangled element types of the label maps


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_surface.hip.txt")


def test_no_scratch_no_spills(report):
    assert report
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)


def test_lds_and_occupancy(report):
    for name, lds in LDS.items():
        for k, r in _find(report, name).items():
            assert r["LDS Size"] == lds, (k, r)
            assert r["VGPRs"] <= 64 and r["Occupancy"] == 8, (k, r)


def test_kernel_instances(report):
    assert len(_find(report, "surf_border_kernel")) == 4 * 2           # element size x (wide loads | peeled)
    for t in ELEMENT:
        for wide in "01":
            assert len(_find(report, f"surf_border_kernelI{t}Lb{wide}EE")) == 1
    for name in LDS:
        if name != "surf_border_kernel":
            assert len(_find(report, name)) == 1, name


def test_no_other_kernel_in_the_translation_unit(report):
    assert all(any(n in k for n in LDS) for k in report), sorted(report)
    assert len(report) == 8 + 5
