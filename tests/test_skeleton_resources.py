"""The skeleton kernels (ptb_skeleton.hip) use no scratch memory and spill nothing; only the thinning kernel holds LDS -- its tile of two
words a row with the halo of STEPS rows and one word, twice for the double buffer, 4 KiB at STEPS = 32 -- as DESIGN.md ("Skeleton") states
with the register figures pinned here.  Read from the compiler's resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

import skeleton_cases as SC
from test_kernel_resources import _find, _report

KERNELS = ("sk_pack_kernel", "sk_thin_kernel", "sk_unpack_kernel", "sk_count_kernel", "sk_finish_kernel")
CELLS = (64 + 2 * SC.STEPS) * (2 + 2)               # the rows of a tile with its halo x the two owned words with one on either side
EXTRA = 264                                         # what the compiler reports beyond the buffers: the "last change" word and the words of the workgroup-wide vote


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_skeleton.hip.txt")


def test_no_scratch_no_spills(report):
    assert report
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)


def test_lds_of_the_thinning_kernel_and_of_nothing_else(report):
    for name in KERNELS:
        if name != "sk_thin_kernel":
            for k, r in _find(report, name).items():
                assert r["LDS Size"] == 0, (k, r)
    for k, r in _find(report, "sk_thin_kernel").items():
        assert r["LDS Size"] == 2 * 4 * CELLS + EXTRA == 4360, (k, r)                   # two buffers of 32-bit words: the figure of DESIGN.md


def test_registers(report):
    for name in ("sk_thin_kernel", "sk_unpack_kernel", "sk_count_kernel", "sk_finish_kernel"):
        for k, r in _find(report, name).items():
            assert r["VGPRs"] <= 64 and r["Occupancy"] >= 8, (k, r)       # (the compiler reports 35 / 28, 19 / 8, 11 and 22)
    for eb in (1, 2, 4):
        for k, r in _find(report, f"sk_pack_kernelILi{eb}E").items():
            assert r["VGPRs"] <= 72 and r["Occupancy"] >= 7, (k, r)       # 32 elements a thread in registers (72 reported)
    for k, r in _find(report, "sk_pack_kernelILi8E").items():
        assert r["VGPRs"] <= 96 and r["Occupancy"] >= 5, (k, r)           # ... of 64 bits each (96 reported)


def test_kernel_instances(report):
    assert len(_find(report, "sk_pack_kernel")) == 4 * 2                  # element size x (16-byte loads | peeled)
    for eb in (1, 2, 4, 8):
        for wide in "01":
            assert len(_find(report, f"sk_pack_kernelILi{eb}ELb{wide}EE")) == 1
    assert len(_find(report, "sk_thin_kernel")) == 2                      # zhang | guo_hall
    for method in "01":
        assert len(_find(report, f"sk_thin_kernelILi{method}EE")) == 1
    assert len(_find(report, "sk_unpack_kernel")) == 2                    # 16-byte stores | peeled
    for wide in "01":
        assert len(_find(report, f"sk_unpack_kernelILb{wide}EE")) == 1
    assert len(_find(report, "sk_count_kernel")) == 1 and len(_find(report, "sk_finish_kernel")) == 1


def test_no_other_kernel_in_the_translation_unit(report):
    assert all(any(n in k for n in KERNELS) for k in report), sorted(report)
    assert all(any(n in k for k in report) for n in KERNELS), sorted(report)
