"""The connected-component kernels (ptb_components.hip) use no scratch memory and spill nothing: a lane's four values, parents and
roots are arrays indexed by unrolled constants only, and the neighbour offsets are unrolled constants too.  Their LDS is what DESIGN.md
("connected components") states: the tile of phase 1 -- 1024 values in the map's element type plus 1024 32-bit parents --, the 1024-slot
tables that fold areas (8 KiB) and statistics (32 KiB) per workgroup, and a few words elsewhere.  Read from the compiler's resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report

KERNELS = ("cc_local_kernel", "cc_seam_kernel", "cc_flatten_kernel", "cc_rank_kernel", "cc_relabel_kernel", "cc_area_kernel", "cc_rewrite_kernel",
           "cc_stats_init_kernel", "cc_stats_kernel", "cc_stats_finish_kernel", "scan_reduce_kernel", "scan_tile_kernel")
ELEMENT = {"h": 1, "s": 2, "i": 4, "x": 8}          # the mangled element types of the label maps


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_components.hip.txt")


def test_no_scratch_no_spills(report):
    assert report
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["VGPRs"] <= 64 and r["Occupancy"] >= 5, (k, r)       # (5: the 32 KiB table of cc_stats_kernel, five workgroups per CU)


def test_lds_is_what_the_design_states(report):
    for k, r in _find(report, "cc_local_kernel").items():
        t = k.split("cc_local_kernelI")[1][0]
        assert r["LDS Size"] == 1024 * (ELEMENT[t] + 4), (k, r)
    for name, lds in (("cc_seam_kernel", 0), ("cc_flatten_kernel", 16), ("cc_rank_kernel", 64), ("cc_relabel_kernel", 0), ("cc_area_kernel", 8192),
                      ("cc_rewrite_kernel", 0), ("cc_stats_init_kernel", 0), ("cc_stats_kernel", 32768), ("cc_stats_finish_kernel", 0),
                      ("scan_reduce_kernel", 32), ("scan_tile_kernel", 32)):
        for k, r in _find(report, name).items():
            assert r["LDS Size"] == lds, (k, r)


def test_kernel_instances(report):
    assert len(_find(report, "cc_local_kernel")) == 4 * 2 * 2 * 2      # element size x (wide loads | peeled) x (faces | all neighbours) x (2-D | 3-D)
    for t in ELEMENT:
        for wide in "01":
            for full in "01":
                for dim3 in "01":
                    assert len(_find(report, f"cc_local_kernelI{t}Lb{wide}ELb{full}ELb{dim3}EE")) == 1
    assert len(_find(report, "cc_seam_kernel")) == 4 * 2 * 2            # element size x neighbourhood x dims
    assert len(_find(report, "cc_rewrite_kernel")) == 4                 # element size
    assert len(_find(report, "cc_stats_kernel")) == 5                   # no values | their element size
    for single in ("cc_flatten_kernel", "cc_rank_kernel", "cc_relabel_kernel", "cc_area_kernel", "cc_stats_init_kernel", "cc_stats_finish_kernel"):
        assert len(_find(report, single)) == 1, single
    assert len(_find(report, "scan_reduce_kernel")) == 2 and len(_find(report, "scan_tile_kernel")) == 2     # 32-bit counts, 64-bit sums


def test_no_other_kernel_in_the_translation_unit(report):
    assert all(any(n in k for n in KERNELS) for k in report), sorted(report)
    assert all(any(n in k for k in report) for n in KERNELS), sorted(report)
