#!/usr/bin/env python3
"""Microbenchmark of the 3-D loop on torch.channels_last_3d model outputs, at the CT geometry of tools/bench_volume_defer.py: a 512^3 volume
cut into 128^3 tiles every 64 voxels (343 tiles), batches of 4.

For C in {3, 4}, fp32 / bf16 model outputs, no TTA / mirror="dhw", the plain accumulating VolumeMerger and the deferred slab merge
(result: argmax uint8 on the slicer window), one IMAGE -- reset(), integrate_batch(_deaugment) over all tiles, merge_crop -- is timed with
device events in three forms:
  dense:       the batches are dense [V*B, C, d, h, w] tensors (the planar kernels)
  native:      the batches are channels_last_3d and are read where they lie (ptb_volume_channels_last.hip)
  copy-first:  the batches are channels_last_3d and y.contiguous() runs inside the timed region before every integrate call -- what the
               loop did to such batches before the native read existed
The forms alternate in one process (dense / native / copy-first / dense / ...) after a warm-up image of each, --repeats times; the median
and the min..max spread of each are reported, the ratios native / copy-first and native / dense, and for each pair whether the difference
of the medians lies beyond the larger spread.  All forms read the same values: a ring of distinct dense tensors and its channels_last_3d
twin (a deferred merger refuses a reused buffer), several GB long, so no pass finds its inputs in the 256 MB Infinity Cache.

Byte model (the traffic each form needs at least; s = sizeof(model output), V = views or 1, vox = voxels of a tile, P = padded volume):
  plain:      n * vox * (V*C*s tile + 4 weight + 8*C volume r/w + 8 norm r/w) + P * 4*(C+1) zero-fill + window * (4*C + 4) + result
  deferred:   n * vox * V*C*s + result
  copy-first: the above + n * vox * V*C*s * 2   (the copy is read and written once more)
GB/s = model bytes / time; "of 8 TB/s" is that rate over the MI355X's HBM peak.

    python tools/bench_volume_channels_last.py [--repeats 5] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12
SHAPE, TILE, STEP, BATCH = (512, 512, 512), 128, 64, 4
FORMS = ("dense", "native", "copy-first")


def one_image(merger, ring, batches, mirror, crop_args, copy_first):
    merger.reset()
    for i, rois in enumerate(batches):
        y = ring[i % len(ring)]
        y = y[:len(rois)] if mirror is None else y[:8 * len(rois)]
        if copy_first:
            y = y.contiguous()
        if mirror is None:
            merger.integrate_batch(y, rois)
        else:
            merger.integrate_batch_deaugment(y, rois, mirror)
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
        sys.exit("bench_volume_channels_last: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd import _native as N
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumeMerger, VolumeSlicer

    dev = torch.device("cuda:0")
    slicer = VolumeSlicer(SHAPE, TILE, STEP)
    n, vox, padded = len(slicer.crops), TILE ** 3, int(np.prod(slicer.target_shape))
    window = int(np.prod(slicer.volume_shape))
    batches = [slicer.crops[b0:b0 + BATCH] for b0 in range(0, n, BATCH)]
    crop_args = ((slicer,), dict(dtype=torch.uint8, argmax=True))
    spec = dict(crop=slicer, dtype=torch.uint8, argmax=True)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"geometry: volume {SHAPE}, tiles {TILE}^3 every {STEP} -> {n} tiles, batches of {BATCH}, result argmax u8; "
        f"{torch.cuda.get_device_name(dev)}; {args.repeats} alternating repeats, median [min..max]")
    gen = torch.Generator(device=dev).manual_seed(0)
    for C in (3, 4):
        for dtype in (torch.float32, torch.bfloat16):
            for mirror in (None, "dhw"):
                V = 1 if mirror is None else 8
                s = torch.empty(0, dtype=dtype).element_size()
                probe = VolumeMerger(slicer.target_shape, C, slicer.weight, device=dev, crops=slicer.crops, defer=True)
                ring_len = (probe.peak_held_tiles + 2 * BATCH) // BATCH + 2          # longer than the custody window: no batch is handed in while held
                del probe
                rings = {"dense": [(torch.rand((V * BATCH, C, TILE, TILE, TILE), device=dev, generator=gen) * 0.8 + 0.1).to(dtype) for _ in range(ring_len)]}
                rings["native"] = [y.contiguous(memory_format=torch.channels_last_3d) for y in rings["dense"]]
                rings["copy-first"] = rings["native"]
                assert all(N.volume_layout(y) == N.LAYOUT_CHANNELS_LAST for y in rings["native"])
                for path in ("plain", "deferred"):
                    kw = dict(crops=slicer.crops, defer=True, result=spec) if path == "deferred" else {}
                    mergers = {form: VolumeMerger(slicer.target_shape, C, slicer.weight, device=dev, **kw) for form in FORMS}

                    def image(form):
                        return one_image(mergers[form], rings[form], batches, mirror, crop_args, form == "copy-first")

                    results = {form: image(form) for form in FORMS}                  # warm-up image (and the one compared below)
                    torch.cuda.synchronize()
                    same = all(torch.equal(results["dense"], results[form]) for form in FORMS)
                    del results
                    times = {form: [] for form in FORMS}
                    for _ in range(args.repeats):
                        for form in FORMS:
                            times[form].append(device_time(lambda: image(form)))
                    tiles_b = n * vox * V * C * s
                    base = tiles_b + window if path == "deferred" else \
                        n * vox * (V * C * s + 4 + 8 * C + 8) + padded * 4 * (C + 1) + window * (4 * C + 4) + window
                    model = {"dense": base, "native": base, "copy-first": base + 2 * tiles_b}
                    tag = f"C={C} {str(dtype)[6:]:8s} {'no TTA' if mirror is None else 'dhw   '} {path:8s}"
                    med = {}
                    for form in FORMS:
                        t = np.array(times[form])
                        med[form] = float(np.median(t))
                        say(f"{tag} {form:10s} {model[form] / 1e9:8.2f} GB  {med[form] * 1e3:8.3f} ms [{t.min() * 1e3:8.3f}..{t.max() * 1e3:8.3f}]  "
                            f"{model[form] / med[form] / 1e9:7.1f} GB/s  {100 * model[form] / med[form] / PEAK:5.1f} % of 8 TB/s")
                    verdicts = []
                    for other in ("copy-first", "dense"):
                        spread = max(np.ptp(times["native"]), np.ptp(times[other]))
                        diff = med["native"] - med[other]
                        where = "beyond" if abs(diff) > spread else "within"
                        verdicts.append(f"native / {other} = {med['native'] / med[other]:.2f}x (difference {diff * 1e3:+.3f} ms, spread {spread * 1e3:.3f} ms: "
                                        f"{where} the spread)")
                    faster = med["native"] < med["copy-first"] and abs(med["native"] - med["copy-first"]) > max(np.ptp(times["native"]), np.ptp(times["copy-first"]))
                    say(f"{tag} {'; '.join(verdicts)}; native beats copy-first: {faster}; same bits: {same}")
                    del mergers
                    torch.cuda.empty_cache()
                del rings
                torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
