#!/usr/bin/env python3
"""Benchmark of the confusion-matrix kernels on one MI355X (utils/metrics.py, csrc/ptb_confusion.hip).

Inputs, seeded and generated here: 5000 x 5000 uint8 pairs (a 4-class blob label map as merge_crop(argmax=True, dtype=torch.uint8) leaves
it against the same map shifted by a few pixels; 4-class uniform noise; a 150-class blob map), a 512^3 uint8 4-class pair, a
[64, 512, 512] batch scored per sample, and [8, C, 512, 512] logits (C = 4, 19; fp32, bf16) against a uint8 target.  The targets carry
an unlabelled border of 255 that ignore_index skips.

Timed, each call from its start to a device synchronise behind its last piece of work, after a warm-up of every side, in rounds that
alternate between the sides (the order inside a round turns over every round):
  (a) confusion_matrix / confusion_matrix_from_logits                          -- one kernel launch, nothing read back
  (b) the torch-op chain a user writes on the device today: idx = t.long() * K + p.long(), masked for ignore_index,
      torch.bincount(idx, minlength=K * K).view(K, K); for logits the same behind logits.argmax(1)
  (c) on the 5000 x 5000 rows: both maps to the host + np.bincount, in rounds of its own (it leaves the GPU idle)
Reported per row: median and spread (max - min) of the repeats, and whether the sides returned the same integers.
THE BAR: (a) beats (b) by more than the larger spread of the two -- required on the blob-map and logits rows; the noise and K = 150
rows are reported whichever way they fall (a row that misses is marked **...**).

    python tools/bench_metrics.py [--repeats 9] [--edge 5000] [--cube 512] [--out profiles/metrics_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LINES = []
HBM_BYTES_PER_S = 6.29e12        # measured float4 copy rate of the MI355X (8.0 TB/s on the datasheet)


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def alternate(sides, repeats, warmup=2):
    """{name: seconds[repeats]}: `warmup` runs of every side, then `repeats` rounds that run the sides one after the other; the order
    inside a round turns over from round to round, so that no side is always the one that follows another one's idle or busy GPU."""
    for _ in range(warmup):
        for fn in sides.values():
            once(fn)
    times = {k: [] for k in sides}
    order = list(sides)
    for r in range(repeats):
        for k in (order if r % 2 == 0 else order[::-1]):
            times[k].append(once(sides[k]))
    return {k: np.array(v) for k, v in times.items()}


def blob_labels(shape, classes, seed, dev):
    """uint8 label map / volume: argmax of `classes` smooth random fields (low-resolution noise, interpolated)."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn((1, classes) + tuple(max(2, s // 128) for s in shape), generator=g).to(dev)
    if len(shape) == 2:
        rows = [F.interpolate(coarse[:, c0:c0 + 16], size=shape, mode="bicubic", align_corners=False)[0] for c0 in range(0, classes, 16)]
        best, arg = None, None
        for i, r in enumerate(rows):                                  # (in slabs of 16 classes: 150 full-size planes are 15 GB)
            v, a = r.max(0)
            a = a + 16 * i
            if best is None:
                best, arg = v, a
            else:
                take = v > best
                best, arg = torch.where(take, v, best), torch.where(take, a, arg)
        return arg.to(torch.uint8)
    full = F.interpolate(coarse, size=shape, mode="trilinear", align_corners=False)[0]
    return torch.cat([full[:, z0:z0 + 64].argmax(0).to(torch.uint8) for z0 in range(0, shape[0], 64)])


def shifted_truth(pred):
    """The ground truth of a benchmark row: the prediction shifted by a few pixels, with an unlabelled border of 255."""
    t = torch.roll(pred, shifts=(3, 5), dims=(-2, -1)).clone()
    t[..., :8, :] = 255
    t[..., :, :8] = 255
    return t


def chain_labels(p, t, K, ignore, per_sample=False):
    idx = t.long() * K + p.long()
    if per_sample:
        B = p.shape[0]
        idx = idx.view(B, -1) + torch.arange(B, device=p.device)[:, None] * (K * K)
        keep = (t != ignore).view(B, -1)
        return torch.bincount(idx[keep], minlength=B * K * K).view(B, K, K)
    return torch.bincount(idx[t != ignore], minlength=K * K).view(K, K)


def fmt(t):
    return f"{np.median(t) * 1e3:10.3f} ms (spread {(t.max() - t.min()) * 1e3:8.3f} ms)"


def verdict(t, required):
    gap = float(np.median(t["b"]) - np.median(t["a"]))
    spread = float(max(t["a"].max() - t["a"].min(), t["b"].max() - t["b"].min()))
    met = gap > spread
    text = f"(b) - (a) = {gap * 1e3:.3f} ms, larger spread {spread * 1e3:.3f} ms: the bar is {'met' if met else 'NOT met'} ((b) / (a) = {np.median(t['b']) / np.median(t['a']):.2f})"
    say("  " + (text if met else f"**{text}**") + ("" if required else "   [reported, not required]"))
    return met


def bench_labels(name, p, t, K, repeats, M, required, per_sample=False, host=False, burst=False):
    say(f"{name}: pred / target {list(p.shape)} uint8, K = {K}, ignore_index = 255{', per sample' if per_sample else ''}")

    def side_a():
        return M.confusion_matrix(p, t, K, ignore_index=255, per_sample=per_sample)

    def side_b():
        return chain_labels(p, t, K, 255, per_sample)

    a, b = side_a(), side_b()
    same = torch.equal(a, b)
    say(f"  {int(a.sum())} positions counted in {int((a != 0).sum())} non-zero cells; (a) == (b): {same}")
    tm = alternate({"a": side_a, "b": side_b}, repeats)
    nbytes = p.numel() * p.element_size() + t.numel() * t.element_size()
    med = float(np.median(tm["a"]))
    say(f"  (a) confusion_matrix           {fmt(tm['a'])}   {nbytes / med / 1e9:8.1f} GB/s of input bytes read once, end to end = "
        f"{100 * nbytes / med / HBM_BYTES_PER_S:.1f} % of the {HBM_BYTES_PER_S / 1e12:.2f} TB/s copy rate")
    say(f"  (b) torch-op chain on device   {fmt(tm['b'])}")
    if burst:                                                         # the stream-ordered form of a validation epoch: out=, no read back
        out = torch.zeros_like(a)

        def many():
            for _ in range(20):
                M.confusion_matrix(p, t, K, ignore_index=255, per_sample=per_sample, out=out)
            return out

        tb = alternate({"x": many}, repeats, warmup=1)["x"] / 20
        say(f"      20 calls with out= behind one synchronise: {np.median(tb) * 1e3:.3f} ms per call (spread {(tb.max() - tb.min()) * 1e3:.3f} ms) = "
            f"{nbytes / np.median(tb) / 1e9:.1f} GB/s = {100 * nbytes / np.median(tb) / HBM_BYTES_PER_S:.1f} % of the copy rate")
    if host:
        def side_c():
            hp, ht = p.cpu().numpy().reshape(-1), t.cpu().numpy().reshape(-1)
            keep = ht != 255
            return np.bincount(ht[keep].astype(np.int64) * K + hp[keep], minlength=K * K).reshape(K, K)

        same = same and np.array_equal(side_c(), a.cpu().numpy())
        tc = alternate({"c": side_c}, max(3, repeats // 3), warmup=1)["c"]
        say(f"  (c) D2H + np.bincount          {fmt(tc)}   ((c) / (a) = {np.median(tc) / med:.0f}); equal: {same}")
    return verdict(tm, required), same


def bench_logits(shape, dtype, repeats, M, dev):
    Nb, C = shape[0], shape[1]
    g = torch.Generator().manual_seed(C)
    coarse = torch.randn((Nb, C, 8, 8), generator=g).to(dev)
    x = (F.interpolate(coarse, size=shape[2:], mode="bicubic", align_corners=False) * 4 + torch.randn(shape, generator=g).to(dev) * 0.3).to(dtype)
    t = shifted_truth(x.argmax(1).to(torch.uint8))
    say(f"logits {list(shape)} {str(dtype).replace('torch.', '')} against a uint8 target, ignore_index = 255")

    def side_a():
        return M.confusion_matrix_from_logits(x, t, ignore_index=255)

    def side_b():
        return chain_labels(x.argmax(1), t, C, 255)

    a, b = side_a(), side_b()
    same = torch.equal(a, b)
    tm = alternate({"a": side_a, "b": side_b}, repeats)
    nbytes = x.numel() * x.element_size() + t.numel()
    med = float(np.median(tm["a"]))
    say(f"  (a) confusion_matrix_from_logits {fmt(tm['a'])}   {nbytes / med / 1e9:8.1f} GB/s of input bytes, end to end; (a) == (b): {same}")
    say(f"  (b) argmax + torch-op chain      {fmt(tm['b'])}")
    return verdict(tm, True), same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--edge", type=int, default=5000)
    ap.add_argument("--cube", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "metrics_bench.txt"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("bench_metrics: at least 7 repeats")
    if not torch.cuda.is_available():
        sys.exit("bench_metrics: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import metrics as M

    dev = torch.device("cuda:0")
    try:
        busy = f"{torch.cuda.utilization(dev)} % busy before the first launch"
    except Exception as e:      # (the query needs the SMI python binding)
        busy = f"load of the GPU before the run unknown ({type(e).__name__}); the spreads below are what other work would show up in"
    say(f"confusion matrices on {torch.cuda.get_device_name(dev)}; {args.repeats} alternating repeats (order reversed every round) after 2 warm-up runs of "
        f"every side; host clock around device-synchronised calls; GPU: {busy}")
    edge, R = args.edge, args.repeats
    required, reported, equal = [], [], []

    p = blob_labels((edge, edge), 4, 0, dev)
    m, s = bench_labels("blob label map", p, shifted_truth(p), 4, R, M, True, host=True, burst=True)
    required.append(m); equal.append(s)
    g2 = torch.Generator().manual_seed(1)
    p = torch.randint(0, 4, (edge, edge), generator=g2, dtype=torch.uint8).to(dev)
    t = torch.randint(0, 4, (edge, edge), generator=g2, dtype=torch.uint8).to(dev)
    t[:8] = 255
    m, s = bench_labels("uniform noise", p, t, 4, R, M, False, host=True, burst=True)
    reported.append(m); equal.append(s)
    p = blob_labels((edge, edge), 150, 3, dev)
    m, s = bench_labels("150-class blob label map", p, shifted_truth(p), 150, R, M, False, burst=True)
    reported.append(m); equal.append(s)
    del p, t
    p = blob_labels((args.cube,) * 3, 4, 2, dev)
    m, s = bench_labels("label volume", p, shifted_truth(p), 4, R, M, True, burst=True)
    required.append(m); equal.append(s)
    p = blob_labels((64 * 512, 512), 4, 4, dev).view(64, 512, 512)
    m, s = bench_labels("batch of label maps", p, shifted_truth(p), 4, R, M, True, per_sample=True)
    required.append(m); equal.append(s)
    del p
    for C in (4, 19):
        for dtype in (torch.float32, torch.bfloat16):
            m, s = bench_logits((8, C, 512, 512), dtype, R, M, dev)
            required.append(m); equal.append(s)
    say(f"all outputs equal: {all(equal)}")
    say("THE BAR ((a) beats (b) by more than the spread on every blob-map and logits row): " + ("met" if all(required) else "**NOT met**"))
    say(f"reported rows (uniform noise, K = 150) beat the chain by more than the spread: {reported}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
