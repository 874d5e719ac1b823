#!/usr/bin/env python3
"""Microbenchmark of the two ends of the 3-D tiled loop on the device: VolumeSlicer.split_device (ptb_volume_split) and
VolumeMerger.merge_crop (ptb_volume_merge_crop), at the CT geometry of a 512^3 volume cut into 128^3 tiles every 64 voxels
(343 tiles), timed with device events.

split:  every tile of the volume in batches of --batch tiles, for int16 C = 1 (CT, Hounsfield units) and uint16 C = 4 (multi-channel
        MR / microscopy) volumes, fp32 and bf16 outputs.  Bytes the algorithm needs: each tile's input voxels read once, its output
        written once (n * d * h * w * C * (sizeof(in) + sizeof(out))).
merge:  merge_crop of the [C, 512, 512, 512] accumulator to the volume, C = 1 and 4, fp32 / bf16 values and the uint8 argmax label
        map, channels first ("cdhw"); for C = 4 also fp32 channels last ("dhwc").  Bytes: the window's C accumulator planes and the normaliser read once, the output written once.

Each configuration is warmed up, then a full pass is timed --repeats times; the median is reported.  GB/s = bytes / time; "of 8 TB/s"
is that rate over the MI355X's HBM peak.  Prints one line per configuration and, with --out, writes them as JSON.

    python tools/bench_volume_edges.py [--batch 4] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12
SHAPE, TILE, STEP = (512, 512, 512), 128, 64


def timed(fn, repeats):
    """Median device time in seconds of fn() over `repeats` runs, after two warm-up runs."""
    for _ in range(2):
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


def row(kind, what, nbytes, seconds):
    r = dict(entry=kind, config=what, bytes=int(nbytes), ms=round(seconds * 1e3, 3), gbps=round(nbytes / seconds / 1e9, 1),
             of_peak=round(nbytes / seconds / PEAK, 3))
    print(f"{kind:6s} {what:38s} {nbytes / 1e9:8.3f} GB  {r['ms']:9.3f} ms  {r['gbps']:8.1f} GB/s  {100 * r['of_peak']:5.1f} % of 8 TB/s", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_volume_edges: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumeMerger, VolumeSlicer

    dev = torch.device("cuda:0")
    slicer = VolumeSlicer(SHAPE, TILE, STEP)
    n = len(slicer.crops)
    tile_vox = TILE ** 3
    print(f"geometry: volume {SHAPE}, tiles {TILE}^3 every {STEP} -> {n} tiles, batches of {args.batch}; "
          f"{torch.cuda.get_device_name(dev)}", flush=True)
    rows = []
    gen = torch.Generator(device=dev).manual_seed(0)
    for in_dtype, C, value in ((torch.int16, 1, -1024), (torch.uint16, 4, 0)):
        shape = SHAPE if C == 1 else SHAPE + (C,)
        vol = torch.randint(0, 4096, shape, device=dev, dtype=torch.int16, generator=gen).view(in_dtype)   # (a view: no uint16 cast kernel needed)
        for out_dtype in (torch.float32, torch.bfloat16):
            def split_pass():
                for b0 in range(0, n, args.batch):
                    slicer.split_device(vol, indices=slice(b0, b0 + args.batch), value=value, dtype=out_dtype)

            nbytes = n * tile_vox * C * (vol.element_size() + torch.empty(0, dtype=out_dtype).element_size())
            rows.append(row("split", f"{str(in_dtype)[6:]} C={C} -> {str(out_dtype)[6:]}", nbytes, timed(split_pass, args.repeats)))
        del vol
        torch.cuda.empty_cache()
    for C in (1, 4):
        merger = VolumeMerger(slicer.target_shape, C, slicer.weight, device=dev)
        merger.volume.uniform_(0, 1, generator=gen)
        merger.norm_mask.uniform_(1, 8, generator=gen)
        vox = int(np.prod(SHAPE))
        configs = (("cdhw -> fp32", dict(dtype=torch.float32), 4 * C), ("cdhw -> bf16", dict(dtype=torch.bfloat16), 2 * C),
                   ("cdhw -> argmax uint8", dict(argmax=True, dtype=torch.uint8), 1))
        if C == 4:
            configs += (("dhwc -> fp32", dict(layout="dhwc", dtype=torch.float32), 4 * C),)
        for label, kw, out_bytes in configs:
            nbytes = vox * (4 * C + 4 + out_bytes)
            rows.append(row("merge", f"C={C} {label}", nbytes, timed(lambda: merger.merge_crop(slicer, **kw), args.repeats)))
        del merger
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(geometry=dict(volume=SHAPE, tile=TILE, step=STEP, tiles=n, batch=args.batch), peak_bytes_per_s=PEAK,
                           device=torch.cuda.get_device_name(dev), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
