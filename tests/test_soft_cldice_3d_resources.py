"""The dims=3 soft-skeleton kernels (ptb_softskel3d.hip) use no scratch memory, spill nothing and hold the LDS blocks their static_asserts
state.  Read from the compiler's resource remarks of the session's forced rebuild."""
from pathlib import Path

from test_kernel_resources import _find, _report


def test_no_scratch_no_spills_and_the_lds_blocks(forced_build):
    report = _report(Path(forced_build["remarks_dir"]) / "ptb_softskel3d.hip.txt")
    assert len(report) == 6 + 1 + 2 and all(k.startswith("_ZN3ptb") and "ss3_" in k for k in report), sorted(report)
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (k, r)
    tile2, tile1 = 4 * 12 * 12 * 36, 4 * 10 * 10 * 34                                          # fp32 blocks on the (8, 8, 32) tile + 2 and + 1
    for k, r in _find(report, "ss3_stage_kernel").items():                                     # <FIRST, LAST, SAVE>: LAST adds 4 waves x 2 doubles
        assert r["LDS Size"] == tile2 + tile1 + (64 if "ELb1ELb" in k else 0) and r["Occupancy"] >= 4, (k, r)
    for k, r in _find(report, "ss3_gather_kernel").items():                                    # v, go, gv and the selection bytes
        assert r["LDS Size"] == tile2 + 2 * tile1 + tile1 // 4 <= 160 * 1024 // 3 and r["Occupancy"] >= 3, (k, r)
    assert _find(report, "ss3_direct_kernel").popitem()[1]["LDS Size"] == 0
