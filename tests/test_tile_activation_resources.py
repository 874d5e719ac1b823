"""The kernels of ptb_tile_activation.hip: per kernel one instance per view set (identity and the five TTA groups) x source dtype for
planar sources, one per source dtype x (vector | element loads) for channels-last ones -- activation, temperature, reduction, C and all
extents are run-time values --, no scratch, no spills, LDS only where views transpose.  Read from the compiler's resource remarks of the
session's forced rebuild.  (The sibling tests show that the planar, band-plan and channels-last units kept their instances.)"""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_tile_activation.hip.txt")


D4 = "ILi8ELi6166440E"      # <NV = 8, CODES_D4, ..>: the only view set with transposing views


@pytest.mark.parametrize("kernel, count, occupancy, d4_occupancy", [
    # planar, 512-thread workgroups (two waves per SIMD each): up to four row-preserving views stay under 128 registers -- two workgroups
    # per CU --; d4 holds 2 x 8 float4 of softmax state next to the eight views in flight and is built for one workgroup per CU
    ("tact_reduce_kernel", 6 * 3, 4, 2),
    ("tact_accum_kernel", 6 * 3, 4, 2),
    ("tact_plan_kernel", 6 * 3, 4, 2),
])
def test_planar_kernels(report, kernel, count, occupancy, d4_occupancy):
    hits = {k: r for k, r in _find(report, kernel).items() if "_cl_" not in k}
    assert len(hits) == count, sorted(hits)
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        if D4 in k:
            assert r["LDS Size"] == 4 * 64 * 32 * 4, (k, r)         # four transposing views x 64 x 32 floats
            assert r["Occupancy"] >= d4_occupancy, (k, r)
        else:
            assert r["LDS Size"] == 0, (k, r)
            assert r["Occupancy"] >= occupancy, (k, r)


@pytest.mark.parametrize("kernel, occupancy", [
    # a lane keeps 16 channels of the view in flight, of the view sum and (accumulate, plan) of the blend: 78 / 133 / 99 registers
    ("tact_cl_reduce_kernel", 6),
    ("tact_cl_accum_kernel", 3),
    ("tact_cl_plan_kernel", 4),
])
def test_channels_last_kernels(report, kernel, occupancy):
    hits = _find(report, kernel)
    assert len(hits) == 3 * 2, sorted(hits)
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0 and r["LDS Size"] == 0, (k, r)
        assert r["Occupancy"] >= occupancy, (k, r)


def test_no_other_kernels_in_the_translation_unit(report):
    assert len(report) == 3 * 18 + 3 * 6, sorted(report)
