"""The reconstruction kernels (ptb_reconstruct.hip) use no scratch memory and spill nothing; the relaxation kernel holds its tile of
32-bit keys with the halo in LDS -- 17 KiB in 2-D, 13.5 KiB in 3-D -- and the init, restage, gather and compare kernels none, as
DESIGN.md ("Reconstruction") states with the register figures pinned here.  Read from the compiler's resource remarks of the session's
forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report

KERNELS = ("rc_init_kernel", "rc_relax_kernel", "rc_restage_kernel", "rc_gather_kernel", "rc_compare_kernel")
CELLS = {2: 66 * 66, 3: 10 * 10 * 34}               # a tile with its halo: 64 x 64, and 8 x 8 x 32
BARRIER_WORDS = 256                                 # the workgroup-wide "did anything change" vote


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_reconstruct.hip.txt")


def test_no_scratch_no_spills(report):
    assert report
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)


def test_lds_of_the_relaxation_kernel_and_of_nothing_else(report):
    for name in KERNELS:
        if name != "rc_relax_kernel":
            for k, r in _find(report, name).items():
                assert r["LDS Size"] == 0, (k, r)
    for dims, cells in CELLS.items():
        for k, r in _find(report, f"rc_relax_kernelILi{dims}E").items():
            assert 4 * cells <= r["LDS Size"] <= 4 * cells + BARRIER_WORDS, (k, r)        # the 32-bit keys of R


def test_registers(report):
    for name in ("rc_init_kernel", "rc_restage_kernel", "rc_gather_kernel", "rc_compare_kernel"):
        for k, r in _find(report, name).items():
            assert r["VGPRs"] <= 40 and r["Occupancy"] >= 8, (k, r)       # (the compiler reports 28, 8, 15 and 14 at most)
    for k, r in _find(report, "rc_relax_kernelILi2E").items():
        assert r["VGPRs"] <= 96 and r["Occupancy"] >= 5, (k, r)           # sixteen positions a thread: values, mask keys, neighbour maxima (96 / 95 reported)
    for k, r in _find(report, "rc_relax_kernelILi3E").items():
        assert r["VGPRs"] <= 72 and r["Occupancy"] >= 7, (k, r)           # (69 / 62 reported)


def test_kernel_instances(report):
    assert len(_find(report, "rc_init_kernel")) == 5 * 2 * 2             # value type x (seed map | none) x (wide loads | peeled)
    for dt in range(5):
        for two in "01":
            for wide in "01":
                assert len(_find(report, f"rc_init_kernelILi{dt}ELb{two}ELb{wide}EE")) == 1
    assert len(_find(report, "rc_relax_kernel")) == 4                    # dims x (minimal | full connectivity)
    for dims in "23":
        for full in "01":
            assert len(_find(report, f"rc_relax_kernelILi{dims}ELb{full}EE")) == 1
    assert len(_find(report, "rc_gather_kernel")) == 5 * 2               # value type x (wide | peeled)
    for dt in range(5):
        for wide in "01":
            assert len(_find(report, f"rc_gather_kernelILi{dt}ELb{wide}EE")) == 1
    for name in ("rc_restage_kernel", "rc_compare_kernel"):             # wide | peeled
        assert len(_find(report, name)) == 2
        for wide in "01":
            assert len(_find(report, f"{name}ILb{wide}EE")) == 1


def test_no_other_kernel_in_the_translation_unit(report):
    assert all(any(n in k for n in KERNELS) for k in report), sorted(report)
    assert all(any(n in k for k in report) for n in KERNELS), sorted(report)
