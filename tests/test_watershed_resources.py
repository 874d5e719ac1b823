"""The watershed kernels (ptb_watershed.hip) use no scratch memory and spill nothing; the two relaxation kernels hold their tile in at
most 64 KiB of LDS -- at least two workgroups per CU -- and the init and gather kernels none, as DESIGN.md ("Watershed") states with the
register figures pinned here.  Read from the compiler's resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report

KERNELS = ("ws_init_kernel", "ws_cost_kernel", "ws_path_kernel", "ws_gather_kernel")
ELEMENT = {"h": 1, "s": 2, "i": 4, "x": 8}          # the mangled element types of the marker maps
CELLS = {2: 66 * 66, 3: 10 * 10 * 34}               # a tile with its halo: 64 x 64, and 8 x 8 x 32
BARRIER_WORDS = 256                                 # the workgroup-wide "did anything change" vote


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_watershed.hip.txt")


def test_no_scratch_no_spills(report):
    assert report
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)


def test_lds_of_the_relaxation_kernels_and_of_nothing_else(report):
    for name in ("ws_init_kernel", "ws_gather_kernel"):
        for k, r in _find(report, name).items():
            assert r["LDS Size"] == 0, (k, r)
    for dims, cells in CELLS.items():
        for k, r in _find(report, f"ws_cost_kernelILi{dims}E").items():
            assert 4 * cells <= r["LDS Size"] <= 4 * cells + BARRIER_WORDS, (k, r)        # the 32-bit cost keys
        for k, r in _find(report, f"ws_path_kernelILi{dims}E").items():
            assert 12 * cells <= r["LDS Size"] <= 12 * cells + BARRIER_WORDS, (k, r)      # the 64-bit path keys and the cost keys
    for name in ("ws_cost_kernel", "ws_path_kernel"):
        for k, r in _find(report, name).items():
            assert r["LDS Size"] <= 64 * 1024, (k, r)


def test_registers(report):
    for name in ("ws_init_kernel", "ws_gather_kernel"):
        for k, r in _find(report, name).items():
            assert r["VGPRs"] <= 40 and r["Occupancy"] >= 8, (k, r)
    for k, r in _find(report, "ws_cost_kernelILi2E").items():
        assert r["VGPRs"] <= 96 and r["Occupancy"] >= 5, (k, r)       # sixteen positions a thread: values, heights, neighbour minima
    for k, r in _find(report, "ws_cost_kernelILi3E").items():
        assert r["VGPRs"] <= 72 and r["Occupancy"] >= 7, (k, r)
    for k, r in _find(report, "ws_path_kernelILi2E").items():
        assert r["VGPRs"] <= 128 and r["Occupancy"] >= 3, (k, r)      # sixteen 64-bit keys; three workgroups per CU by LDS
    for k, r in _find(report, "ws_path_kernelILi3E").items():
        assert r["VGPRs"] <= 144 and r["Occupancy"] >= 3, (k, r)


def test_kernel_instances(report):
    assert len(_find(report, "ws_init_kernel")) == 5 * 4 * 2           # height type x marker size x (wide loads | peeled)
    for ht in range(5):
        for t in ELEMENT:
            for wide in "01":
                assert len(_find(report, f"ws_init_kernelILi{ht}E{t}Lb{wide}EE")) == 1
    for name in ("ws_cost_kernel", "ws_path_kernel"):                  # dims x (minimal | full connectivity)
        assert len(_find(report, name)) == 4
        for dims in "23":
            for full in "01":
                assert len(_find(report, f"{name}ILi{dims}ELb{full}EE")) == 1
    assert len(_find(report, "ws_gather_kernel")) == 4 * 2             # marker size x (wide | peeled)
    for t in ELEMENT:
        for wide in "01":
            assert len(_find(report, f"ws_gather_kernelI{t}Lb{wide}EE")) == 1


def test_no_other_kernel_in_the_translation_unit(report):
    assert all(any(n in k for n in KERNELS) for k in report), sorted(report)
    assert all(any(n in k for k in report) for n in KERNELS), sorted(report)
