#!/usr/bin/env python3
"""Microbenchmark of resample_volume (one launch of ptb_volume_resize_trilinear), timed with device events on one MI355X:
int16 512^3 -> float32 768^3 (x 1.5: a CT scan brought to a finer model spacing) against what torch offers,
F.interpolate(v.float()[None, None], mode="trilinear").

Reported: the median ms of both sides over --repeats runs that alternate between them after a warm-up of each, the run-to-run spread
(max - min of the repeats), the bytes the algorithm needs (the volume read once, the result written once) and their share of 8 TB/s
at the fused side's time, and torch.cuda.max_memory_allocated of one run of each side (inputs included).  Before that the agreement of
the two sides on these inputs, within the tolerance of tests/test_volume_resample_gpu.py: tol = 4 d + 1e-7 with d the deviation of the
kernel's float32 arithmetic from float64 arithmetic, measured here on a 32^3 -> 48^3 corner of the same volume (the same scales); the
two float32 evaluations of the same taps may differ by 2 tol.  Every step is announced before it starts.

If torch's own trilinear kernel cannot run at the full size, the edge is halved and the output says so.

    python tools/bench_volume_resample.py [--edge 512] [--repeats 7] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def alternate(fused, composed, repeats):
    """Device times in seconds of both sides: two warm-up runs of each, then `repeats` rounds that run one after the other."""
    def once(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        del out
        return start.elapsed_time(stop) * 1e-3

    for _ in range(2):
        once(fused)
        once(composed)
    a, b = [], []
    for _ in range(repeats):
        a.append(once(fused))
        b.append(once(composed))
    return np.array(a), np.array(b)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated()


def report(name, nbytes, fused, composed, repeats, saved_bytes):
    a, b = alternate(fused, composed, repeats)
    ma, mb = float(np.median(a)), float(np.median(b))
    sa, sb = float(a.max() - a.min()), float(b.max() - b.min())
    pa, pb = peak_of(fused), peak_of(composed)
    say(f"{name}")
    say(f"  fused     {ma * 1e3:9.3f} ms (spread {sa * 1e3:.3f} ms)   {nbytes / 1e9:6.2f} GB needed -> {nbytes / ma / 1e9:7.1f} GB/s, "
        f"{100 * nbytes / ma / PEAK:5.1f} % of 8 TB/s   peak memory {pa / 1e9:6.2f} GB")
    say(f"  composed  {mb * 1e3:9.3f} ms (spread {sb * 1e3:.3f} ms)   {'':41s}   peak memory {pb / 1e9:6.2f} GB")
    faster = mb - ma > max(sa, sb)
    say(f"  fused is {mb / ma:.2f}x the composed speed; the difference {(mb - ma) * 1e3:.3f} ms is "
        f"{'more' if faster else 'NOT more'} than the spread; peak memory lower by {(pb - pa) / 1e9:.2f} GB "
        f"({'at least' if pb - pa >= saved_bytes else 'LESS than'} the {saved_bytes / 1e9:.2f} GB intermediate it no longer makes)")
    return faster and pb - pa >= saved_bytes


def restatement_d(q, size):
    """Largest deviation of the kernels' float32 arithmetic (taps in float32; x, then y, then z; every product and sum rounded) from the
    same taps in float64 arithmetic, on float32 values q [C, d, h, w] (align_corners = False)."""
    def blend(x, dtype):
        for axis in (3, 2, 1):
            n_in, n_out = x.shape[axis], size[axis - 1]
            scale = np.float32(n_in / n_out)
            src = np.maximum(scale * (np.arange(n_out, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
            i0 = np.minimum(src.astype(np.int64), n_in - 1)
            i1 = i0 + (i0 < n_in - 1)
            lam = np.clip(src - i0.astype(np.float32), 0, 1).astype(np.float32)
            shape = [1, 1, 1, 1]
            shape[axis] = -1
            x = np.take(x, i0, axis=axis) * (np.float32(1) - lam).astype(dtype).reshape(shape) + np.take(x, i1, axis=axis) * lam.astype(dtype).reshape(shape)
        return x

    return float(np.abs(blend(q.astype(np.float32), np.float32).astype(np.float64) - blend(q.astype(np.float64), np.float64)).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edge", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_volume_resample: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.inference.tiles_3d import resample_volume

    dev = torch.device("cuda:0")
    edge = args.edge
    gen = torch.Generator(device=dev).manual_seed(0)
    while True:
        size = (edge * 3 // 2,) * 3
        try:
            probe = F.interpolate(torch.zeros((1, 1, edge, edge, edge), device=dev), size=size, mode="trilinear")
            torch.cuda.synchronize()
            del probe
            break
        except RuntimeError as e:
            say(f"torch's trilinear kernel cannot run at {edge}^3 -> {size[0]}^3 on this machine ({str(e).splitlines()[0]}): the edge is halved")
            edge //= 2
    vox_in, vox_out = edge ** 3, size[0] ** 3
    say(f"geometry: int16 [{edge}^3] -> float32 [{size[0]}^3]; {args.repeats} alternating repeats; {torch.cuda.get_device_name(dev)}")
    ct = torch.randint(-1024, 3072, (edge,) * 3, device=dev, dtype=torch.int16, generator=gen)
    torch.cuda.synchronize()
    say("one fused call ...")
    got = resample_volume(ct, size)
    torch.cuda.synchronize()
    say("one composed call ...")
    ref = F.interpolate(ct.float()[None, None], size=size, mode="trilinear")[0, 0]
    torch.cuda.synchronize()
    dv = restatement_d(ct[:32, :32, :32].float().cpu().numpy()[None], (48, 48, 48))
    worst = float((got - ref).abs().max())
    del got, ref
    say(f"agreement: d = {dv:.3g} on Hounsfield-like values; max |fused - composed| = {worst:.3g} (allowed 2 (4 d + 1e-7) = {2 * (4 * dv + 1e-7):.3g})")
    ok = worst <= 2 * (4 * dv + 1e-7)
    say("timing ...")
    ok &= report(f"resample_volume int16 [{edge}^3] -> float32 [{size[0]}^3]", 2 * vox_in + 4 * vox_out,
                 lambda: resample_volume(ct, size), lambda: F.interpolate(ct.float()[None, None], size=size, mode="trilinear")[0, 0],
                 args.repeats, 4 * vox_in)
    say("all conditions hold" if ok else "NOT all conditions hold")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
