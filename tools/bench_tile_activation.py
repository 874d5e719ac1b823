#!/usr/bin/env python3
"""Microbenchmark of ``activation=`` in the 2-D tile merges (ptb_tile_activation.hip) at the headline geometry of bench.py: a 5000 x 5000
image cut into 512 x 512 tiles every 256 pixels, batches of 8 tiles, C = 4 logits, ``merge()`` as the result.

Rows: {deferred, incremental} x {no TTA, d4} x {fp32, bf16} x {dense, channels_last} x {sigmoid, softmax}.  Every row times one IMAGE
(reset, all integrate calls, merge) with device events, three ways:
  (a) fused:    integrate_batch(_deaugment)(y, crops, .., activation=..)
  (b) unfused:  p = y.float().softmax(1) | .sigmoid() by torch, then today's integrate_batch(_deaugment)(p, crops, ..) -- code this tree
                shares with its parent commit
  (c) none:     today's call on the raw logits, no activation at all (what the arithmetic of (a) costs on top: a / c)
The three are run in one process, alternating a / b / c after a warm-up image of each, --repeats times; the median and the min..max of
each are reported.  The bar: (a) is faster than (b) by more than the larger of their two spreads.  `peak MB` = the allocator's peak above
the ring of model outputs during the warm-up image (accumulators or result, and for (b) the probability tensors torch writes -- with a
deferred merger those are what is held).  All three read the same ring of distinct batches (a deferred merger refuses a reused buffer),
longer than the custody window and several GB, so no pass finds its inputs in the 256 MB Infinity Cache.

    python tools/bench_tile_activation.py [--repeats 3] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IMAGE, TILE, STEP, BATCH, C = (5000, 5000), 512, 256, 8, 4


def probabilities(y, activation):
    z = y.float()
    return z.softmax(1) if activation == "softmax" else z.sigmoid()


def one_image(merger, ring, batches, group, how, activation):
    merger.reset()
    V = 1 if group is None else 8
    for i, crops in enumerate(batches):
        y = ring[i % len(ring)][:V * len(crops)]
        kw = dict(activation=activation) if how == "fused" else {}
        if how == "unfused":
            y = probabilities(y, activation)
        if group is None:
            merger.integrate_batch(y, crops, **kw)
        else:
            merger.integrate_batch_deaugment(y, crops, group, **kw)
    return merger.merge()


def device_time(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tile_activation: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer, TileMerger

    dev = torch.device("cuda:0")
    slicer = ImageSlicer(IMAGE + (3,), TILE, STEP, weight="pyramid")
    n = len(slicer.crops)
    batches = [slicer.crops[b0:b0 + BATCH] for b0 in range(0, n, BATCH)]
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"geometry: image {IMAGE}, tiles {TILE}^2 every {STEP} -> {n} tiles, batches of {BATCH}, C = {C}, result merge() fp32; "
        f"{torch.cuda.get_device_name(dev)}; {args.repeats} alternating repeats, median [min..max] ms")
    probe = TileMerger(slicer.target_shape, C, slicer.weight, device=dev, crops=slicer.crops, defer=True)
    ring_len = (probe._bands.peak_tiles() + 2 * BATCH) // BATCH + 2          # longer than the custody window: no batch is handed in while held
    del probe
    gen = torch.Generator(device=dev).manual_seed(0)
    missed = []
    for group in (None, "d4"):
        V = 1 if group is None else 8
        for dtype in (torch.float32, torch.bfloat16):
            for layout in ("dense", "channels_last"):
                ring = []
                for _ in range(min(ring_len, len(batches))):
                    y = (torch.rand((V * BATCH, C, TILE, TILE), device=dev, generator=gen) * 6 - 3).to(dtype)
                    ring.append(y.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else y)
                    del y
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                base = torch.cuda.memory_allocated()
                for path in ("deferred", "incremental"):
                    for activation in ("sigmoid", "softmax"):
                        kw = dict(crops=slicer.crops, defer=True) if path == "deferred" else dict(auto_plan=False)
                        merger = TileMerger(slicer.target_shape, C, slicer.weight, device=dev, **kw)
                        hows = ("fused", "unfused", "none")
                        peaks, maps = {}, {}
                        for how in hows:          # warm-up image, its peak memory, and the maps compared below
                            torch.cuda.synchronize()
                            torch.cuda.reset_peak_memory_stats()
                            maps[how] = one_image(merger, ring, batches, group, how, activation).clone()
                            torch.cuda.synchronize()
                            peaks[how] = torch.cuda.max_memory_allocated() - base
                        differ = float((maps["fused"] - maps["unfused"]).abs().nan_to_num(0.0).max())
                        del maps
                        times = {how: [] for how in hows}
                        for _ in range(args.repeats):
                            for how in hows:
                                times[how].append(device_time(lambda: one_image(merger, ring, batches, group, how, activation)))
                        t = {how: np.array(times[how]) * 1e3 for how in hows}
                        med = {how: float(np.median(t[how])) for how in hows}
                        spread = max(float(np.ptp(t["fused"])), float(np.ptp(t["unfused"])))
                        ok = med["unfused"] - med["fused"] > spread
                        tag = f"{path:11s} {'no TTA' if group is None else 'd4    '} {str(dtype)[6:]:8s} {layout:13s} {activation:7s}"
                        say(f"{tag} (a) fused {med['fused']:8.3f} [{t['fused'].min():8.3f}..{t['fused'].max():8.3f}] peak {peaks['fused'] / 1e6:8.1f} MB | "
                            f"(b) unfused {med['unfused']:8.3f} [{t['unfused'].min():8.3f}..{t['unfused'].max():8.3f}] peak {peaks['unfused'] / 1e6:8.1f} MB | "
                            f"(c) none {med['none']:8.3f} [{t['none'].min():8.3f}..{t['none'].max():8.3f}] | b / a = {med['unfused'] / med['fused']:5.2f}x, "
                            f"a / c = {med['fused'] / med['none']:5.2f}x, spread {spread:.3f} ms: {'a beats b' if ok else 'MISSES THE BAR'}; "
                            f"max |a - b| = {differ:.2e}; mode {merger.mode}")
                        if not ok:
                            missed.append(tag)
                        del merger
                        torch.cuda.empty_cache()
                del ring
                torch.cuda.empty_cache()
    say(f"rows that miss the bar (a faster than b by more than the spread): {len(missed)}" + "".join(f"\n  {m}" for m in missed))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
