"""band_pair_kernel (csrc/ptb_bandpair.hip) keeps two covering tiles' worth of loads in registers -- the one being reduced and the one in
flight -- and both halves' LDS tiles: one 1024-thread workgroup per CU, so 128 registers and 128 KiB of LDS are all it can have, and a
build that spills is not acceptable (scratch in the band kernel once cost 20 %).  Read from the session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report


@pytest.fixture(scope="module")
def remarks(forced_build):
    return Path(forced_build["remarks_dir"])


def test_band_pair_kernel_fits_one_workgroup_per_cu(remarks):
    hits = _find(_report(remarks / "ptb_bandpair.hip.txt"), "band_pair_kernel")
    assert len(hits) == 4, sorted(hits)                        # linear / non-linear reduction x fp16 / bf16
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["VGPRs"] <= 128 and r["LDS Size"] <= 128 * 1024 and r["Occupancy"] >= 4, (k, r)
