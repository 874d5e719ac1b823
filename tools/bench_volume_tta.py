#!/usr/bin/env python3
"""Microbenchmark of mirror test-time augmentation in the 3-D tiled loop, at the CT geometry of tools/bench_volume_edges.py: a 512^3
volume cut into 128^3 tiles every 64 voxels (343 tiles), batches of 4 tiles x 8 views (mirror="dhw"), timed with device events.

merge:  one full pass of de-augment + blend over all 343 tiles, for C = 1 and 4 and fp32 / bf16 model outputs:
        (a) the torch-op loop: y = torch.stack([c.flip(dims) for c in y.chunk(8)]).mean(0); merger.integrate_batch(y, rois)
        (b) merger.integrate_batch(mirror_volume_deaugment(y, "dhw"), rois)
        (c) merger.integrate_batch_deaugment(y, rois, "dhw")
split:  the model input of every tile of an int16 C = 1 volume as fp32 / bf16: split_device without views, split_device(mirror="dhw"),
        and split_device followed by mirror_volume_augment.

Byte model (the traffic each variant needs at least; s = sizeof(model output), per output voxel of a tile):
  (c) V*C*s views read + 8*C + 8 accumulator and normaliser read and written + 4 weight;
  (b) (c) + C*s de-augmented tile written and read again (+ 8*C for the float32 copy integrate_batch makes of a bf16 tile);
  (a) (b) + 4*V*C*s: every view is flipped into a copy and the copies are stacked (read + write each).
  split: n * d*h*w * (sizeof(in) + V * sizeof(out)); split + augment adds n * d*h*w * 2 * sizeof(out).
Each configuration is warmed up, then a full pass is timed --repeats times; the median is reported.  GB/s = model bytes / time; "of
8 TB/s" is that rate over the MI355X's HBM peak.  Prints one line per configuration and, with --out, writes them as JSON.

    python tools/bench_volume_tta.py [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12
SHAPE, TILE, STEP, BATCH = (512, 512, 512), 128, 64, 4
FLIPS = {0: [], 1: [4], 2: [3], 3: [3, 4], 4: [2], 5: [2, 4], 6: [2, 3], 7: [2, 3, 4]}


def timed(fn, repeats):
    """Median device time in seconds of fn() over `repeats` runs, after one warm-up run."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) * 1e-3)
    return float(np.median(times))


def row(kind, what, nbytes, seconds, rows):
    r = dict(entry=kind, config=what, bytes=int(nbytes), ms=round(seconds * 1e3, 3), gbps=round(nbytes / seconds / 1e9, 1),
             of_peak=round(nbytes / seconds / PEAK, 3))
    print(f"{kind:6s} {what:44s} {nbytes / 1e9:8.3f} GB  {r['ms']:9.3f} ms  {r['gbps']:8.1f} GB/s  {100 * r['of_peak']:5.1f} % of 8 TB/s", flush=True)
    rows.append(r)
    return seconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_volume_tta: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.inference import MIRROR_VIEWS, mirror_volume_augment, mirror_volume_deaugment
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumeMerger, VolumeSlicer

    dev = torch.device("cuda:0")
    slicer = VolumeSlicer(SHAPE, TILE, STEP)
    n = len(slicer.crops)
    views = MIRROR_VIEWS["dhw"]
    V = len(views)
    vox = TILE ** 3
    print(f"geometry: volume {SHAPE}, tiles {TILE}^3 every {STEP} -> {n} tiles, batches of {BATCH} tiles x {V} views; "
          f"{torch.cuda.get_device_name(dev)}", flush=True)
    rows, speedups = [], []
    gen = torch.Generator(device=dev).manual_seed(0)
    batches = [slicer.crops[b0:b0 + BATCH] for b0 in range(0, n, BATCH)]
    for C in (1, 4):
        merger = VolumeMerger(slicer.target_shape, C, slicer.weight, device=dev)
        for dtype in (torch.float32, torch.bfloat16):
            s = torch.empty(0, dtype=dtype).element_size()
            y = (torch.rand((V * BATCH, C, TILE, TILE, TILE), device=dev, generator=gen) + 0.5).to(dtype)   # stand-in model output

            def torch_ops():
                for rois in batches:
                    yy = y[:V * len(rois)]
                    t = torch.stack([c.flip(FLIPS[m]) if FLIPS[m] else c for c, m in zip(yy.chunk(V), views)]).mean(0)
                    merger.integrate_batch(t, rois)

            def unfused():
                for rois in batches:
                    merger.integrate_batch(mirror_volume_deaugment(y[:V * len(rois)], "dhw"), rois)

            def fused():
                for rois in batches:
                    merger.integrate_batch_deaugment(y[:V * len(rois)], rois, "dhw")

            fused_b = V * C * s + 8 * C + 8 + 4
            unfused_b = fused_b + 2 * C * s + (8 * C if s == 2 else 0)
            torch_b = unfused_b + 4 * V * C * s
            tag = f"C={C} {str(dtype)[6:]}"
            ta = row("merge", f"{tag} (a) torch ops", n * vox * torch_b, timed(torch_ops, args.repeats), rows)
            tb = row("merge", f"{tag} (b) deaugment + integrate_batch", n * vox * unfused_b, timed(unfused, args.repeats), rows)
            tc = row("merge", f"{tag} (c) integrate_batch_deaugment", n * vox * fused_b, timed(fused, args.repeats), rows)
            speedups.append(dict(config=tag, a_over_c=round(ta / tc, 2), b_over_c=round(tb / tc, 2)))
            print(f"       {tag}: (a) / (c) = {ta / tc:.2f}x, (b) / (c) = {tb / tc:.2f}x", flush=True)
            del y
        del merger
        torch.cuda.empty_cache()
    vol = torch.randint(0, 4096, SHAPE, device=dev, dtype=torch.int16, generator=gen)
    for dtype in (torch.float32, torch.bfloat16):
        s = torch.empty(0, dtype=dtype).element_size()

        def split_plain():
            for b0 in range(0, n, BATCH):
                slicer.split_device(vol, indices=slice(b0, b0 + BATCH), value=-1024, dtype=dtype)

        def split_mirror():
            for b0 in range(0, n, BATCH):
                slicer.split_device(vol, indices=slice(b0, b0 + BATCH), value=-1024, dtype=dtype, mirror="dhw")

        def split_then_augment():
            for b0 in range(0, n, BATCH):
                mirror_volume_augment(slicer.split_device(vol, indices=slice(b0, b0 + BATCH), value=-1024, dtype=dtype), "dhw")

        tag = f"int16 C=1 -> {str(dtype)[6:]}"
        row("split", f"{tag}", n * vox * (2 + s), timed(split_plain, args.repeats), rows)
        row("split", f"{tag} mirror=dhw", n * vox * (2 + V * s), timed(split_mirror, args.repeats), rows)
        row("split", f"{tag} split + mirror_volume_augment", n * vox * (2 + V * s + 2 * s), timed(split_then_augment, args.repeats), rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(geometry=dict(volume=SHAPE, tile=TILE, step=STEP, tiles=n, batch=BATCH, views=V), peak_bytes_per_s=PEAK,
                           device=torch.cuda.get_device_name(dev), rows=rows, speedups=speedups), f, indent=1)


if __name__ == "__main__":
    main()
