"""The run-length codec's kernels (ptb_rle.hip) use no scratch memory, spill nothing and keep their LDS far below the 40 KB that lets four
workgroups share a CU: a lane's four per-column counters / offsets and its chunk of rows are arrays indexed by unrolled constants only,
and the launch's labels are picked out of the by-value argument with a select chain.  Read from the compiler's resource remarks of the
session's forced rebuild."""
from pathlib import Path

import pytest

from test_kernel_resources import _find, _report

KERNELS = ("rle_pass_kernel", "scan_reduce_kernel", "scan_tile_kernel", "rle_enc_offsets_kernel", "rle_lengths_kernel", "rle_fill_kernel",
           "rle_transpose_kernel")


@pytest.fixture(scope="module")
def report(forced_build):
    return _report(Path(forced_build["remarks_dir"]) / "ptb_rle.hip.txt")


def test_no_scratch_no_spills_small_lds(report):
    assert report
    for k, r in report.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] <= 40 * 1024, (k, r)


def test_pass_kernel_instances(report):
    hits = _find(report, "rle_pass_kernel")
    assert len(hits) == 4 * 2 * 2                    # element size x (wide loads | peeled) x (count | write)
    for k, r in hits.items():
        assert r["LDS Size"] == 0, (k, r)
        if "rle_pass_kernelIh" in k:                  # the 1-byte masks of merge_crop(argmax=True, dtype=torch.uint8)
            assert r["VGPRs"] <= 64 and r["Occupancy"] >= 8, (k, r)
    assert _find(report, "rle_transpose_kernel").popitem()[1]["LDS Size"] == 64 * 68


def test_no_other_kernel_in_the_translation_unit(report):
    assert all(any(n in k for n in KERNELS) for k in report), sorted(report)
    assert all(any(n in k for k in report) for n in KERNELS), sorted(report)
