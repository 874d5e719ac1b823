"""The band kernels sum their normaliser in registers instead of loading it (csrc/ptb_bandplan.hip and the three kernels that share
its work-item table): the accumulator must not push an instance over a register cliff.  A plain-loop instance that crossed 64 VGPRs
(8 waves per SIMD -> 7) once cost 10 % (profiles/HISTORY.md section 9.5), so every ``band_plan_kernel`` instance that was at or below
64 before the normaliser moved into the kernel -- the names in tests/golden/band_plan_kernel_le64_vgprs.json, read from the compiler's
resource remarks of that build -- still is; none of the kernels has scratch.  Read from the session's forced rebuild."""
import json
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report

GOLDEN = Path(__file__).parent / "golden" / "band_plan_kernel_le64_vgprs.json"


@pytest.fixture(scope="module")
def remarks(forced_build):
    return Path(forced_build["remarks_dir"])


def test_band_plan_instances_stay_below_their_register_cliff(remarks):
    hits = _find(_report(remarks / "ptb_bandplan.hip.txt"), "band_plan_kernel")
    assert len(hits) == 156, len(hits)
    for k, r in hits.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
    small = json.loads(GOLDEN.read_text())
    assert len(small) == 120 and set(small) <= set(hits), sorted(set(small) - set(hits))
    for k in small:
        assert hits[k]["VGPRs"] <= 64 and hits[k]["Occupancy"] >= 8, (k, hits[k])


def test_sibling_plan_kernels_have_no_scratch(remarks):
    """tact_plan_kernel / tact_cl_plan_kernel (fused activation) and cl_plan_kernel (channels_last): the same rule, the same budget."""
    act = _report(remarks / "ptb_tile_activation.hip.txt")
    last = _report(remarks / "ptb_channels_last.hip.txt")
    found = {**_find(act, "tact_plan_kernel"), **_find(act, "tact_cl_plan_kernel"), **_find(last, "cl_plan_kernel")}
    assert len(found) == 18 + 6 + 12, len(found)
    for k, r in found.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
