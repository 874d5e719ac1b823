#!/usr/bin/env python3
"""Microbenchmark of the front of the 2-D tiled loop on the device: ImageSlicer.split_device (ptb_split_tiles) at the headline
geometry (cfg2: a 5000 x 5000 image, tiles of 512 every 256 -> 361 tiles, batches of 8 tiles with d4 TTA, i.e. 64 output tiles per
call), timed with device events.

Cases: the uint8 x 3 -> fp32 constant-border call of the first device split, 16-bit multispectral images (uint16 x 4), half-precision
batches (bf16) and the REFLECT_101 border, plus the cases that isolate one change at a time (uint16 x 3, uint8 REFLECT_101,
uint16 x 4 constant -> bf16).  Bytes the algorithm needs per call: the 8 tiles' input pixels read once (n * th * tw * C * sizeof(in)) and
the 8 x 8 augmented views written once (V * n * C * th * tw * sizeof(out)).

Each case is warmed up, then a pass over the first 360 tiles (45 calls of 8 tiles) is timed --repeats times; the median pass divided
by the number of calls is the time per call.  Prints one line per case and, with --out, writes them as JSON.

    python tools/bench_split_device.py [--repeats 9] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12
SHAPE, TILE, STEP, BATCH, AUGMENT, VIEWS = (5000, 5000), 512, 256, 8, "d4", 8
CONSTANT, REFLECT_101 = 0, 4
# (label, image dtype, channels, border, output dtype)
CASES = [
    ("u8x3 -> fp32 CONSTANT", torch.uint8, 3, CONSTANT, torch.float32),
    ("u16x4 -> fp32 CONSTANT", torch.uint16, 4, CONSTANT, torch.float32),
    ("u8x3 -> bf16 CONSTANT", torch.uint8, 3, CONSTANT, torch.bfloat16),
    ("u16x4 -> bf16 REFLECT_101", torch.uint16, 4, REFLECT_101, torch.bfloat16),
    ("u16x3 -> fp32 CONSTANT", torch.uint16, 3, CONSTANT, torch.float32),
    ("u8x3 -> fp32 REFLECT_101", torch.uint8, 3, REFLECT_101, torch.float32),
    ("u16x4 -> bf16 CONSTANT", torch.uint16, 4, CONSTANT, torch.bfloat16),
]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_split_device: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer

    dev = torch.device("cuda:0")
    slicer = ImageSlicer(SHAPE, TILE, STEP)
    n = len(slicer.crops)
    calls = n // BATCH
    print(f"geometry: image {SHAPE}, tiles {TILE} every {STEP} -> {n} tiles, {calls} calls of {BATCH} tiles x {VIEWS} views ({AUGMENT}); "
          f"{torch.cuda.get_device_name(dev)}", flush=True)
    gen = torch.Generator(device=dev).manual_seed(0)
    rows = []
    for label, in_dtype, C, border, out_dtype in CASES:
        # (uint16: a view of random int16 bits -- every value of the type, no uint16 cast kernel needed)
        img = torch.randint(-32768, 32768, SHAPE + (C,), device=dev, dtype=torch.int16, generator=gen)
        img = img.view(torch.uint16) if in_dtype == torch.uint16 else (img & 255).to(torch.uint8)

        def split_pass():
            for b0 in range(0, calls * BATCH, BATCH):
                slicer.split_device(img, slice(b0, b0 + BATCH), augment=AUGMENT, border_type=border, dtype=out_dtype)

        seconds = timed(split_pass, args.repeats) / calls
        isz, osz = img.element_size(), torch.empty(0, dtype=out_dtype).element_size()
        nbytes = BATCH * TILE * TILE * C * (isz + VIEWS * osz)
        r = dict(config=label, in_dtype=str(in_dtype)[6:], channels=C, border=border, out_dtype=str(out_dtype)[6:], bytes_per_call=int(nbytes),
                 us_per_call=round(seconds * 1e6, 2), gbps=round(nbytes / seconds / 1e9, 1), of_peak=round(nbytes / seconds / PEAK, 3))
        print(f"{label:28s} {nbytes / 1e6:8.1f} MB/call  {r['us_per_call']:8.2f} us/call  {r['gbps']:8.1f} GB/s  "
              f"{100 * r['of_peak']:5.1f} % of 8 TB/s", flush=True)
        rows.append(r)
        del img
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(geometry=dict(image=SHAPE, tile=TILE, step=STEP, tiles=n, batch=BATCH, augment=AUGMENT, calls=calls),
                           peak_bytes_per_s=PEAK, device=torch.cuda.get_device_name(dev), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
