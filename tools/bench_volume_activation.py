#!/usr/bin/env python3
"""Microbenchmark of ``activation=`` in the 3-D tile merges (ptb_volume_activation.hip) at the CT geometry of tools/bench_volume_defer.py:
a 512^3 volume cut into 128^3 tiles every 64 voxels (343 tiles), batches of 4, C = 4 logits, argmax-uint8 result.

Rows: {deferred, accumulating} x {no TTA, mirror="dhw"} x {fp32, bf16} x {dense, channels_last_3d} with softmax, and sigmoid on the deferred
rows.  Every row times one IMAGE (reset, all integrate calls, merge_crop) with device events, three ways:
  (a) fused:    integrate_batch(_deaugment)(y, rois, .., activation=..)
  (b) unfused:  p = y.float().softmax(1) | .sigmoid() by torch, then today's integrate_batch(_deaugment)(p, rois, ..) -- code this tree shares
                with its parent commit
  (c) none:     today's call on the raw logits, no activation at all (what the arithmetic of (a) costs on top: a / c)
The three are run in one process, alternating a / b / c after a warm-up image of each, --repeats times; the median and the min..max of
each are reported.  The bar: (a) is faster than (b) by more than the larger of their two spreads.  `peak MB` = the allocator's peak above
the ring of model outputs during the warm-up image (accumulators or result, the plan table, and for (b) the probability tensors torch
writes -- with a deferred merger those are what is held).  All three read the same ring of distinct batches (a deferred merger refuses a
reused buffer), longer than the custody window and several GB, so no pass finds its inputs in the 256 MB Infinity Cache.

    python tools/bench_volume_activation.py [--repeats 3] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE, TILE, STEP, BATCH, C = (512, 512, 512), 128, 64, 4, 4


def probabilities(y, activation):
    z = y.float()
    return z.softmax(1) if activation == "softmax" else z.sigmoid()


def one_image(merger, ring, batches, mirror, slicer, how, activation):
    merger.reset()
    V = 1 if mirror is None else 8
    for i, rois in enumerate(batches):
        y = ring[i % len(ring)][:V * len(rois)]
        kw = dict(activation=activation) if how == "fused" else {}
        if how == "unfused":
            y = probabilities(y, activation)
        if mirror is None:
            merger.integrate_batch(y, rois, **kw)
        else:
            merger.integrate_batch_deaugment(y, rois, mirror, **kw)
    return merger.merge_crop(slicer, dtype=torch.uint8, argmax=True)


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
        sys.exit("bench_volume_activation: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumeMerger, VolumeSlicer

    dev = torch.device("cuda:0")
    slicer = VolumeSlicer(SHAPE, TILE, STEP)
    n = len(slicer.crops)
    batches = [slicer.crops[b0:b0 + BATCH] for b0 in range(0, n, BATCH)]
    spec = dict(crop=slicer, dtype=torch.uint8, argmax=True)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"geometry: volume {SHAPE}, tiles {TILE}^3 every {STEP} -> {n} tiles, batches of {BATCH}, C = {C}, result argmax uint8; "
        f"{torch.cuda.get_device_name(dev)}; {args.repeats} alternating repeats, median [min..max] ms")
    probe = VolumeMerger(slicer.target_shape, C, slicer.weight, device=dev, crops=slicer.crops, defer=True)
    ring_len = (probe.peak_held_tiles + 2 * BATCH) // BATCH + 2          # longer than the custody window: no batch is handed in while held
    del probe
    gen = torch.Generator(device=dev).manual_seed(0)
    missed = []
    for mirror in (None, "dhw"):
        V = 1 if mirror is None else 8
        for dtype in (torch.float32, torch.bfloat16):
            for layout in ("dense", "channels_last_3d"):
                ring = []
                for _ in range(ring_len):
                    y = (torch.rand((V * BATCH, C, TILE, TILE, TILE), device=dev, generator=gen) * 6 - 3).to(dtype)
                    ring.append(y.contiguous(memory_format=torch.channels_last_3d) if layout == "channels_last_3d" else y)
                    del y
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                base = torch.cuda.memory_allocated()
                for path, activation in (("deferred", "softmax"), ("deferred", "sigmoid"), ("accumulating", "softmax")):
                    kw = dict(crops=slicer.crops, defer=True, result=spec) if path == "deferred" else {}
                    merger = VolumeMerger(slicer.target_shape, C, slicer.weight, device=dev, **kw)
                    hows = ("fused", "unfused", "none")
                    peaks, labels = {}, {}
                    for how in hows:          # warm-up image, its peak memory, and the labels compared below
                        torch.cuda.synchronize()
                        torch.cuda.reset_peak_memory_stats()
                        labels[how] = one_image(merger, ring, batches, mirror, slicer, how, activation)
                        torch.cuda.synchronize()
                        peaks[how] = torch.cuda.max_memory_allocated() - base
                    differ = float((labels["fused"] != labels["unfused"]).float().mean())
                    del labels
                    times = {how: [] for how in hows}
                    for _ in range(args.repeats):
                        for how in hows:
                            times[how].append(device_time(lambda: one_image(merger, ring, batches, mirror, slicer, how, activation)))
                    t = {how: np.array(times[how]) * 1e3 for how in hows}
                    med = {how: float(np.median(t[how])) for how in hows}
                    spread = max(float(np.ptp(t["fused"])), float(np.ptp(t["unfused"])))
                    ok = med["unfused"] - med["fused"] > spread
                    tag = f"{path:12s} {'no TTA' if mirror is None else 'dhw   '} {str(dtype)[6:]:8s} {layout:16s} {activation:7s}"
                    say(f"{tag} (a) fused {med['fused']:8.3f} [{t['fused'].min():8.3f}..{t['fused'].max():8.3f}] peak {peaks['fused'] / 1e6:8.1f} MB | "
                        f"(b) unfused {med['unfused']:8.3f} [{t['unfused'].min():8.3f}..{t['unfused'].max():8.3f}] peak {peaks['unfused'] / 1e6:8.1f} MB | "
                        f"(c) none {med['none']:8.3f} [{t['none'].min():8.3f}..{t['none'].max():8.3f}] | b / a = {med['unfused'] / med['fused']:5.2f}x, "
                        f"a / c = {med['fused'] / med['none']:5.2f}x, spread {spread:.3f} ms: {'a beats b' if ok else 'MISSES THE BAR'}; "
                        f"labels of a and b differ on {100 * differ:.4f} % of the voxels")
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
