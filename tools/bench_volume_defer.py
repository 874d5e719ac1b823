#!/usr/bin/env python3
"""Microbenchmark of the deferred slab merge, VolumeMerger(crops=, defer=True, result=), against the plain accumulating path of the same
tree, at the CT geometry of tools/bench_volume_tta.py: a 512^3 volume cut into 128^3 tiles every 64 voxels (343 tiles), batches of 4.

For C in {1, 4}, fp32 / bf16 model outputs, no TTA / mirror="dhw", result argmax-uint8 / float32, one IMAGE is timed with device events:
  plain:    reset() (zero volume and norm_mask), integrate_batch(_deaugment) over all tiles, merge_crop(slicer, ...)
  deferred: reset() (a fresh result tensor), the same integrate calls, merge_crop(slicer, ...) (returns what the slabs wrote)
The two are run in one process, alternating plain / deferred / plain / deferred after a warm-up image of each, --repeats times; the
median and the min..max spread of each are reported, and their ratio.  Both read the same batches: a ring of distinct tensors (a deferred
merger refuses a reused buffer), several GB long, so no pass finds its inputs in the 256 MB Infinity Cache.

Byte model (the traffic each path needs at least; s = sizeof(model output), V = views or 1, vox = voxels of a tile, P = padded volume):
  plain:    n * vox * (V*C*s tile + 4 weight + 8*C volume r/w + 8 norm r/w) + P * 4*(C+1) zero-fill + window * (4*C + 4) + result
  deferred: n * vox * V*C*s + result      (the 8 MB weight window stays in cache)
GB/s = model bytes / time; "of 8 TB/s" is that rate over the MI355X's HBM peak.  Memory: `extra MB` = the allocator's peak above the
ring during an image (accumulators, table, result) plus the model outputs alive at once -- one batch for the plain path, the most
bytes in custody for the deferred one (in a real loop those are live model outputs, not a preallocated ring).

    python tools/bench_volume_defer.py [--repeats 5] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12
SHAPE, TILE, STEP, BATCH = (512, 512, 512), 128, 64, 4


def one_image(merger, ring, batches, mirror, crop_args):
    merger.reset()
    for i, rois in enumerate(batches):
        y = ring[i % len(ring)]
        if mirror is None:
            merger.integrate_batch(y[:len(rois)], rois)
        else:
            merger.integrate_batch_deaugment(y[:8 * len(rois)], rois, mirror)
    return merger.merge_crop(*crop_args[0], **crop_args[1])


def device_time(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_volume_defer: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumeMerger, VolumeSlicer

    dev = torch.device("cuda:0")
    slicer = VolumeSlicer(SHAPE, TILE, STEP)
    n, vox, padded = len(slicer.crops), TILE ** 3, int(np.prod(slicer.target_shape))
    window = int(np.prod(slicer.volume_shape))
    batches = [slicer.crops[b0:b0 + BATCH] for b0 in range(0, n, BATCH)]
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"geometry: volume {SHAPE}, tiles {TILE}^3 every {STEP} -> {n} tiles, batches of {BATCH}; {torch.cuda.get_device_name(dev)}; "
        f"{args.repeats} alternating repeats, median [min..max]")
    gen = torch.Generator(device=dev).manual_seed(0)
    for C in (1, 4):
        for dtype in (torch.float32, torch.bfloat16):
            for mirror in (None, "dhw"):
                V = 1 if mirror is None else 8
                s = torch.empty(0, dtype=dtype).element_size()
                probe = VolumeMerger(slicer.target_shape, C, slicer.weight, device=dev, crops=slicer.crops, defer=True)
                ring_len = (probe.peak_held_tiles + 2 * BATCH) // BATCH + 2          # longer than the custody window: no batch is handed in while held
                del probe
                ring = [(torch.rand((V * BATCH, C, TILE, TILE, TILE), device=dev, generator=gen) * 0.9 + 0.05).to(dtype) for _ in range(ring_len)]
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                for out_dtype, argmax, out_b in ((torch.uint8, True, 1), (torch.float32, False, 4 * C)):
                    crop_args = ((slicer,), dict(dtype=out_dtype, argmax=argmax))
                    spec = dict(crop=slicer, dtype=out_dtype, argmax=argmax)
                    results, peaks = {}, {}
                    mergers = {}
                    for path in ("plain", "deferred"):
                        torch.cuda.reset_peak_memory_stats()
                        kw = dict(crops=slicer.crops, defer=True, result=spec) if path == "deferred" else {}
                        mergers[path] = VolumeMerger(slicer.target_shape, C, slicer.weight, device=dev, **kw)
                        results[path] = one_image(mergers[path], ring, batches, mirror, crop_args)      # warm-up image (and the one compared below)
                        torch.cuda.synchronize()
                        peaks[path] = torch.cuda.max_memory_allocated() - base
                        if path == "plain":
                            del mergers[path]          # its 2.7 GB of accumulators are not part of the deferred path's peak
                            torch.cuda.empty_cache()
                    same = torch.equal(results["plain"], results["deferred"])
                    del results
                    mergers["plain"] = VolumeMerger(slicer.target_shape, C, slicer.weight, device=dev)
                    one_image(mergers["plain"], ring, batches, mirror, crop_args)
                    # custody of the deferred path, image by image the same: the most bytes held after any call (an untimed pass)
                    m = mergers["deferred"]
                    m.reset()
                    custody = 0
                    for i, rois in enumerate(batches):
                        y = ring[i % ring_len]
                        if mirror is None:
                            m.integrate_batch(y[:len(rois)], rois)
                        else:
                            m.integrate_batch_deaugment(y[:8 * len(rois)], rois, mirror)
                        custody = max(custody, sum(r[0].numel() * r[0].element_size() for r in m._held))
                    times = {"plain": [], "deferred": []}
                    for _ in range(args.repeats):
                        for path in ("plain", "deferred"):
                            times[path].append(device_time(lambda: one_image(mergers[path], ring, batches, mirror, crop_args)))
                    model = {"plain": n * vox * (V * C * s + 4 + 8 * C + 8) + padded * 4 * (C + 1) + window * (4 * C + 4) + window * out_b,
                             "deferred": n * vox * V * C * s + window * out_b}
                    extra = {"plain": peaks["plain"] + V * BATCH * C * vox * s, "deferred": peaks["deferred"] + custody}
                    tag = f"C={C} {str(dtype)[6:]:8s} {'no TTA' if mirror is None else 'dhw   '} -> {'argmax u8' if argmax else 'float32  '}"
                    med = {}
                    for path in ("plain", "deferred"):
                        t = np.array(times[path])
                        med[path] = float(np.median(t))
                        say(f"{tag} {path:8s} {model[path] / 1e9:8.2f} GB  {med[path] * 1e3:8.3f} ms [{t.min() * 1e3:7.3f}..{t.max() * 1e3:7.3f}]  "
                            f"{model[path] / med[path] / 1e9:7.1f} GB/s  {100 * model[path] / med[path] / PEAK:5.1f} % of 8 TB/s  extra {extra[path] / 1e6:9.1f} MB")
                    spread = max(np.ptp(times["plain"]), np.ptp(times["deferred"]))
                    gain = med["plain"] - med["deferred"]
                    say(f"{tag} plain / deferred = {med['plain'] / med['deferred']:.2f}x (difference {gain * 1e3:+.3f} ms, spread {spread * 1e3:.3f} ms: "
                        f"{'beyond' if abs(gain) > spread else 'within'} the spread); same bits: {same}")
                    del mergers
                    torch.cuda.empty_cache()
                del ring
                torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
