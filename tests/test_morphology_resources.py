"""The morphology kernels (ptb_morphology.hip) use no scratch memory and spill nothing, and the LDS of the two walks is what the header's
constants give -- the levels of a row and the accumulator ring, 55296 bytes for the largest grey instance, so two workgroups share the
160 KiB of a CU ("Morphology").  Read from the compiler's resource remarks of the session's forced rebuild."""
from pathlib import Path

import pytest

from pytorch_toolbelt_amd.utils import morphology as MO
from test_kernel_resources import _find, _report

LEVELS = 6


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_morphology.hip.txt")


def test_no_scratch_no_spills_and_the_lds_of_the_walks(report):
    assert len(report) == 5 * 4 + 5 * 3                                   # grey: dtype x ring; bit planes: (plane | element size) x ring
    for k, r in report.items():
        assert "morph_walk_kernel" in k or "morph_bits_kernel" in k, k
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
    for ring in (4, 16, 32, 64):
        hits = _find(report, "morph_walk_kernel", f"ELi{ring}EE")
        assert len(hits) == 5
        for k, r in hits.items():
            assert r["LDS Size"] == 4 * (LEVELS * (MO.STRIP + 64) + ring * MO.STRIP), (k, r)
            assert 2 * r["LDS Size"] <= 160 * 1024 and r["VGPRs"] <= 64, (k, r)
    for ring in (4, 16, 64):
        hits = _find(report, "morph_bits_kernel", f"ELi{ring}EE")
        assert len(hits) == 5
        for k, r in hits.items():
            assert r["LDS Size"] == 4 * (LEVELS * (MO.BIT_WORDS + 2 + 2) + ring * (MO.BIT_WORDS + 2)), (k, r)
