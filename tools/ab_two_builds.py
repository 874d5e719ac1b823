#!/usr/bin/env python3
"""Same-process A/B of TWO BUILDS of libptb_hip.so on the headline band merge.

Which physical memory backs the 12 GB of model outputs moves the step by up to 15 % from one process to the next and by 9 % between
pools of one process (profiles/r04_placement_pmc.md section 1), while one pool of one process repeats to 0.2 %.  A kernel change worth
a few per cent can therefore only be seen when both builds run in ONE process on the SAME buffers.  This tool loads two libraries by
path with ctypes (neither is the package's own: nothing of pytorch_toolbelt_amd._native is involved) and drives the same band plan
through each one's C ABI -- ptb_band_plan_create, ptb_band_plan_upload, then per image ptb_band_plan_reset and one
ptb_band_plan_submit per batch (46 at the headline geometry) -- on the same batch tensors, window, normaliser and output map,
alternating A, B, A, B ... with a pair of HIP events around every image.  That is repeated over K candidate pools of model outputs,
allocated one after the other and all kept, as the placement study did.  Per pool: median and spread (interquartile range, and min /
max) of each build's images, the difference of the medians set against three times the larger spread, and whether the two maps are
equal bit for bit.

    python tools/ab_two_builds.py --a build/parent/libptb_hip.so --b pytorch_toolbelt_amd/lib/libptb_hip.so --dtype fp32 --views d4

The parent's library comes from a checkout of the parent commit: ``python -c "import __graft_entry__ as g; g.build(out_dir=DIR)"``."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VP, I64, INT = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
DTYPES = {"fp32": (torch.float32, 0), "fp16": (torch.float16, 1), "bf16": (torch.bfloat16, 2)}
RED_SUM, RED_MEAN = 0, 1


class Build:
    """One libptb_hip.so and its band plan of the geometry."""

    def __init__(self, path, name):
        self.name, self.path = name, os.path.abspath(path)
        lib = self.lib = ctypes.CDLL(self.path)
        lib.ptb_band_plan_create.restype = I64
        lib.ptb_band_plan_create.argtypes = [VP, VP, INT, INT, INT, INT, INT, INT, INT, INT, INT, VP, INT, VP]
        lib.ptb_band_plan_upload.argtypes = [VP, VP, VP]
        lib.ptb_band_plan_reset.argtypes = [VP]
        lib.ptb_band_plan_destroy.argtypes = [VP]
        lib.ptb_band_plan_destroy.restype = None
        lib.ptb_band_plan_submit.argtypes = [VP, INT, INT, VP, I64, I64, INT, INT, VP, INT, VP, VP, VP, VP]
        lib.ptb_norm_accumulate.argtypes = [VP, VP, VP, VP, INT, INT, INT, INT, INT, VP, INT, VP]
        self.handle = self.table = None

    def plan(self, xs, ys, C, th, tw, H, W, rows, dev, stream):
        handle = VP()
        nbytes = self.lib.ptb_band_plan_create(xs.ctypes.data, ys.ctypes.data, len(xs), C, th, tw, H, W, rows, 0, H, None, 0, ctypes.byref(handle))
        if nbytes < 0:
            raise SystemExit(f"{self.name}: ptb_band_plan_create returned {nbytes}")
        self.handle = handle
        self.table = torch.empty(max(int(nbytes), 64), dtype=torch.uint8, device=dev)
        rc = self.lib.ptb_band_plan_upload(handle, self.table.data_ptr(), stream)
        if rc < 0:
            raise SystemExit(f"{self.name}: ptb_band_plan_upload returned {rc}")

    def image(self, batches, sizes, per_tile, dcode, varr, n_views, red, merged, norm, weight, stream):
        """One image: every batch of the pool through ptb_band_plan_submit; returns the launches issued."""
        lib, handle = self.lib, self.handle
        lib.ptb_band_plan_reset(handle)
        pos = launches = 0
        for t, B in zip(batches, sizes):
            rc = lib.ptb_band_plan_submit(handle, pos, B, t.data_ptr(), per_tile, B * per_tile, dcode, n_views, varr, red, merged, norm, weight, stream)
            if rc < 0:
                raise SystemExit(f"{self.name}: ptb_band_plan_submit returned {rc} at tile {pos}")
            pos += B
            launches += rc
        return launches

    def close(self):
        if self.handle:
            self.lib.ptb_band_plan_destroy(self.handle)
            self.handle = None


def iqr(values):
    q = statistics.quantiles(values, n=4)
    return q[2] - q[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--a", required=True, help="libptb_hip.so of build A (the parent)")
    ap.add_argument("--b", required=True, help="libptb_hip.so of build B (the candidate)")
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="fp32", help="element type of the model outputs")
    ap.add_argument("--views", choices=["d4", "identity"], default="d4", help="d4: eight views per tile, mean; identity: the loop without TTA")
    ap.add_argument("--pools", type=int, default=6, help="candidate pools of model outputs, all kept allocated")
    ap.add_argument("--images", type=int, default=24, help="timed images per build and pool (alternating A, B)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=2, default=(5000, 5000))
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--step", type=int, default=256)
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8, help="tiles per batch")
    ap.add_argument("--rows", type=int, default=1024, help="rows per launch group")
    ap.add_argument("--json", help="also write the per-pool records to this file")
    args = ap.parse_args()

    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer
    from pytorch_toolbelt_amd.inference.tta import DEAUGMENT_VIEWS

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    stream = VP(torch.cuda.current_stream(dev).cuda_stream)
    slicer = ImageSlicer(tuple(args.shape) + (3,), args.tile, args.step, weight="pyramid")
    crops = np.asarray(slicer.crops, dtype=np.int64)
    H, W = (int(v) for v in slicer.target_shape)
    n, C, th, tw = len(crops), args.channels, args.tile, args.tile
    xs, ys = np.ascontiguousarray(crops[:, 0]), np.ascontiguousarray(crops[:, 1])
    views = list(DEAUGMENT_VIEWS["d4"]) if args.views == "d4" else [0]
    n_views, red = len(views), (RED_MEAN if args.views == "d4" else RED_SUM)
    varr = (ctypes.c_int * n_views)(*views)
    tdtype, dcode = DTYPES[args.dtype]
    sizes = [min(args.batch, n - b0) for b0 in range(0, n, args.batch)]
    per_tile = C * th * tw

    builds = [Build(args.a, "A"), Build(args.b, "B")]
    weight = torch.from_numpy(np.ascontiguousarray(slicer.weight, dtype=np.float32)).to(dev).reshape(1, th, tw).contiguous()
    norm = torch.zeros((1, H, W), device=dev)
    rc = builds[0].lib.ptb_norm_accumulate(norm.data_ptr(), weight.data_ptr(), xs.ctypes.data, ys.ctypes.data, n, th, tw, H, W, None, 0, stream)
    if rc < 0:
        raise SystemExit(f"ptb_norm_accumulate returned {rc}")
    merged = torch.empty((C, H, W), device=dev)
    for b in builds:
        b.plan(xs, ys, C, th, tw, H, W, args.rows, dev, stream)
    torch.cuda.synchronize()
    print(f"A = {builds[0].path}\nB = {builds[1].path}")
    print(f"{args.shape[0]} x {args.shape[1]}, tile {th}, step {args.step}, C = {C}, {args.views} ({n_views} view(s)), {args.dtype}: {n} tiles in {len(sizes)} "
          f"submits per image, {n * n_views * per_tile * torch.empty(0, dtype=tdtype).element_size() / 1e9:.2f} GB of model outputs per pool")

    g = torch.Generator(device=dev).manual_seed(0)
    pools, records = [], []
    for k in range(args.pools):
        pools.append([torch.randn((n_views * B, C, th, tw), device=dev, generator=g).to(tdtype) for B in sizes])      # (kept: the next pool lands elsewhere)
    ptrs = (merged.data_ptr(), norm.data_ptr(), weight.data_ptr())
    for k, pool in enumerate(pools):
        ms = {b.name: [] for b in builds}
        launches = {}
        for i in range(args.warmup + args.images):
            for b in builds:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launches[b.name] = b.image(pool, sizes, per_tile, dcode, varr, n_views, red, *ptrs, stream)
                e1.record()
                e1.synchronize()
                if i >= args.warmup:
                    ms[b.name].append(e0.elapsed_time(e1))
        maps = []
        for b in builds:
            merged.fill_(-1.0)
            b.image(pool, sizes, per_tile, dcode, varr, n_views, red, *ptrs, stream)
            maps.append(merged.clone())
        same = bool(torch.equal(maps[0].view(torch.int32), maps[1].view(torch.int32)))
        del maps
        med = {nm: statistics.median(v) for nm, v in ms.items()}
        spread = {nm: iqr(v) for nm, v in ms.items()}
        gain = med["A"] - med["B"]
        bar = 3 * max(spread.values())
        verdict = "B faster" if gain > bar else ("B SLOWER" if -gain > bar else "no difference")
        rec = dict(pool=k, first_batch=hex(pool[0].data_ptr()), launches=launches, median_ms=med, iqr_ms=spread,
                   min_ms={nm: min(v) for nm, v in ms.items()}, max_ms={nm: max(v) for nm, v in ms.items()}, gain_ms=gain,
                   gain_pct=100 * gain / med["A"], three_spreads_ms=bar, verdict=verdict, maps_equal=same)
        records.append(rec)
        print(f"pool {k} @{rec['first_batch']}: A {med['A']:.4f} ms (iqr {spread['A']:.4f}, {rec['min_ms']['A']:.4f}..{rec['max_ms']['A']:.4f})   "
              f"B {med['B']:.4f} ms (iqr {spread['B']:.4f}, {rec['min_ms']['B']:.4f}..{rec['max_ms']['B']:.4f})   "
              f"A - B = {gain:+.4f} ms ({rec['gain_pct']:+.2f} %) against 3 x spread = {bar:.4f}: {verdict}; maps equal: {same}", flush=True)
    for b in builds:
        b.close()
    out = dict(a=builds[0].path, b=builds[1].path, dtype=args.dtype, views=args.views, shape=list(args.shape), tile=th, step=args.step, channels=C,
               images=args.images, pools=records)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(out, open(args.json, "w"), indent=1)
    print(json.dumps(dict(faster=sum(r["verdict"] == "B faster" for r in records), slower=sum(r["verdict"] == "B SLOWER" for r in records),
                          same=sum(r["verdict"] == "no difference" for r in records), maps_equal=all(r["maps_equal"] for r in records),
                          mean_gain_pct=sum(r["gain_pct"] for r in records) / len(records))))


if __name__ == "__main__":
    main()
