#!/usr/bin/env python
"""Generate tests/golden/rle.npz: what the UNMODIFIED reference's utils/rle.py returns for the seeded masks of tests/rle_cases.py.

Test infrastructure only.  Run where a checkout of the reference exists, named by PTB_REFERENCE:

    PTB_REFERENCE=<reference checkout> python tools/make_rle_golden.py

The reference's module is loaded from its file (its package __init__ would pull in cv2 and torchvision); no reference source is copied.
Recorded per case: rle_encode(mask), rle_to_string of it, and (two-valued masks) the bit-packed rle_decode of that string; once, the
decode of runs that overlap and come out of order.  The masks themselves are not stored: the tests rebuild them from pattern, shape
and seed.
"""
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rle_cases as RC  # noqa: E402


def main():
    ref_root = os.environ.get("PTB_REFERENCE")
    if not ref_root:
        raise SystemExit("set PTB_REFERENCE to a checkout of the unmodified reference (the directory holding pytorch_toolbelt/)")
    spec = importlib.util.spec_from_file_location("_reference_rle", os.path.join(ref_root, "pytorch_toolbelt", "utils", "rle.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    arrays, cases = {}, []
    for case in RC.GOLDEN_CASES:
        mask = RC.case_mask(case)
        assert max(mask.shape) <= 300
        runs = ref.rle_encode(mask)
        text = ref.rle_to_string(runs)
        entry = dict(case, string=text, two_valued=bool(len(np.unique(mask[mask != 0])) <= 1), run_dtype=str(runs.dtype))
        arrays[case["name"] + "/rle"] = runs
        if entry["two_valued"]:
            decoded = ref.rle_decode(text, mask.shape, np.uint8)
            assert np.array_equal(decoded, mask), case["name"]                     # the reference round-trips its own encoding
            arrays[case["name"] + "/decoded_bits"] = np.packbits(np.ascontiguousarray(decoded))
        cases.append(entry)
    text = ref.rle_to_string(RC.OVERLAP_RUNS)
    arrays["overlap/decoded_bits"] = np.packbits(np.ascontiguousarray(ref.rle_decode(text, RC.OVERLAP_SHAPE, np.uint8)))
    arrays["overlap/decoded_bool_bits"] = np.packbits(np.ascontiguousarray(ref.rle_decode(text, RC.OVERLAP_SHAPE, np.bool_)))
    arrays["__cases__"] = np.array(json.dumps(cases))
    arrays["__overlap__"] = np.array(json.dumps({"runs": RC.OVERLAP_RUNS, "shape": list(RC.OVERLAP_SHAPE), "string": text}))
    np.savez_compressed(RC.GOLDEN, **arrays)
    print(f"{RC.GOLDEN}: {len(cases)} cases, {os.path.getsize(RC.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
