"""The dims=3 skeleton kernels (ptb_skeleton3d.hip) use no scratch memory and spill nothing; only the thinning kernel holds LDS -- the brick
with its halo and a word on either side in x, twice (the state and the candidates of the pass) -- as the unit's constants say.  Read from
the compiler's resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from pytorch_toolbelt_amd.utils import skeleton as S
from test_kernel_resources import _find, _report

KERNELS = ("sk3_pack_kernel", "sk3_thin_kernel")
CELLS = (S.BRICK[0] + 2 * S.HALO) * (S.BRICK[1] + 2 * S.HALO) * (S.BRICK[2] // 32 + 2)
EXTRA = 264                                         # as for the plane unit: the "last change" word and the words of the workgroup-wide vote


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_skeleton3d.hip.txt")


def test_no_scratch_no_spills_and_no_other_kernel(report):
    assert report and all(any(n in k for n in KERNELS) for k in report), sorted(report)
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
    assert len(_find(report, "sk3_pack_kernel")) == 4 * 2 and len(_find(report, "sk3_thin_kernel")) == 1


def test_lds_of_the_thinning_kernel_and_of_nothing_else(report):
    for k, r in _find(report, "sk3_pack_kernel").items():
        assert r["LDS Size"] == 0, (k, r)
    for k, r in _find(report, "sk3_thin_kernel").items():
        assert S.HALO == 9 * S.PASSES and r["LDS Size"] == 2 * 4 * CELLS + EXTRA, (k, r)
        assert r["Occupancy"] >= 4, (k, r)                                     # four workgroups of four waves a CU within its 160 KB of LDS
