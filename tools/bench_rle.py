#!/usr/bin/env python3
"""Benchmark of the run-length codec on one MI355X (utils/rle.py, csrc/ptb_rle.hip).

Inputs, seeded and generated here: a 5000 x 5000 uint8 4-class blob label map (what merge_crop(argmax=True, dtype=torch.uint8) leaves
on the device), a 5000 x 5000 50 % noise mask, and a [512, 512, 512] 4-class blob label volume encoded slice by slice.

Timed, each call from its start to a device synchronise behind its last piece of work (every side ends in host-visible sizes, so a
host clock around synchronised work is the honest one), after a warm-up of every side, in rounds that alternate between the sides
(the order inside a round turns over every round; the host side (c) has rounds of its own, because a device side timed right behind
its 0.1 s of host-only work measures a GPU that has gone idle: (a) took 0.46-0.55 ms in that position, 0.18-0.25 ms otherwise):
  (a) rle_encode_device(mask, labels=...)                                       -- the kernels, one D2H of 8 bytes per encoding
  (b) the torch-op chain a user would write on the device today, per label:    (m == c).T.flatten(), pad, compare, nonzero, subtract
  (c) mask.cpu() + this project's host rle_encode, per label
  (d) rle_decode_device(device runs) against the host rle_decode(runs) + H2D of the mask
Reported per input: median and spread (max - min) of the repeats, mask bytes over the time of (a) -- an end-to-end rate of a
latency- and launch-bound call, not a share of any peak --, and whether all sides returned the same integers.
THE BAR: (a) beats (b) by more than the larger spread of the two, on both 2-D inputs.

    python tools/bench_rle.py [--repeats 7] [--edge 5000] [--cube 512] [--out profiles/rle_bench.txt]
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


def torch_chain(fg):
    """What a user writes with torch ops on the device: the encoding of a boolean [H, W] foreground map."""
    f = fg.T.flatten()
    padded = F.pad(f, (1, 1))
    edges = torch.nonzero(padded[1:] != padded[:-1]).flatten() + 1
    edges[1::2] -= edges[0::2]
    return edges


def blob_labels(shape, classes, seed, dev):
    """uint8 label map / volume: argmax of `classes` smooth random fields (low-resolution noise, interpolated)."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn((1, classes) + tuple(max(2, s // 128) for s in shape), generator=g).to(dev)
    full = F.interpolate(coarse, size=shape, mode="bicubic" if len(shape) == 2 else "trilinear", align_corners=False)[0]
    if len(shape) == 2:
        return full.argmax(0).to(torch.uint8)
    out = torch.cat([full[:, z0:z0 + 64].argmax(0).to(torch.uint8) for z0 in range(0, shape[0], 64)])      # (in slabs: int64 indices of 512^3 are 1 GB)
    return out


def fmt(t):
    return f"{np.median(t) * 1e3:10.3f} ms (spread {(t.max() - t.min()) * 1e3:8.3f} ms)"


def bench_2d(name, mask, labels, repeats, R):
    """labels: a list (foreground mask == c per label) or None (foreground mask != 0)."""
    H, W = mask.shape
    fgs = (lambda m: [m != 0]) if labels is None else (lambda m: [m == c for c in labels])

    def side_a():
        return R.rle_encode_device(mask, labels=labels)

    def side_b():
        return [torch_chain(fg) for fg in fgs(mask)]

    def side_c():
        host = mask.cpu().numpy()
        return [R.rle_encode(fg.astype(np.uint8)) for fg in fgs(host)]

    say(f"{name}: [{H}, {W}] {str(mask.dtype).replace('torch.', '')}, {'mask != 0' if labels is None else f'labels {list(labels)}'}")
    a, b, c = side_a(), side_b(), side_c()
    a = [a] if labels is None else a
    same = all(torch.equal(x, y) and np.array_equal(x.cpu().numpy(), z) for x, y, z in zip(a, b, c))
    entries = sum(int(x.numel()) for x in a)
    say(f"  {entries} output entries ({entries // 2} runs) in {len(a)} encodings; (a) == (b) == (c): {same}")
    t = alternate({"a": side_a, "b": side_b}, repeats)               # the two device sides against each other ...
    t.update(alternate({"c": side_c}, repeats, warmup=1))            # ... the host side apart: it leaves the GPU idle for 0.1 s per run
    say(f"  (a) rle_encode_device          {fmt(t['a'])}   {mask.numel() * mask.element_size() / np.median(t['a']) / 1e9:8.2f} GB/s of mask bytes, end to end")
    say(f"  (b) torch-op chain on device   {fmt(t['b'])}")
    say(f"  (c) D2H + host rle_encode      {fmt(t['c'])}")
    gap = float(np.median(t["b"]) - np.median(t["a"]))
    spread = float(max(t["a"].max() - t["a"].min(), t["b"].max() - t["b"].min()))
    met = gap > spread
    say(f"  (b) - (a) = {gap * 1e3:.3f} ms, larger spread {spread * 1e3:.3f} ms: the bar is {'met' if met else 'NOT met'} "
        f"((b) / (a) = {np.median(t['b']) / np.median(t['a']):.2f}, (c) / (a) = {np.median(t['c']) / np.median(t['a']):.2f})")

    # (d) decode of the first encoding
    runs = a[0]
    runs_host = runs.cpu().numpy()
    want = fgs(mask)[0].to(torch.uint8)

    def side_d_dev():
        return R.rle_decode_device(runs, (H, W))

    def side_d_host():
        return torch.from_numpy(np.ascontiguousarray(R.rle_decode(runs_host, (H, W), np.uint8))).to(mask.device)

    same_d = torch.equal(side_d_dev(), want) and torch.equal(side_d_host(), want)
    td = alternate({"dev": side_d_dev, "host": side_d_host}, repeats)
    say(f"  (d) rle_decode_device          {fmt(td['dev'])}   of {runs.numel() // 2} runs; both equal the mask: {same_d}")
    say(f"      host rle_decode + H2D      {fmt(td['host'])}")
    return met, same and same_d


def bench_stack(vol, labels, repeats, R):
    B, H, W = vol.shape

    def side_a():
        return R.rle_encode_device(vol, labels=labels)

    def side_b():
        return [[torch_chain(vol[z] == c) for c in labels] for z in range(B)]

    def side_c():
        host = vol.cpu().numpy()
        return [[R.rle_encode((host[z] == c).astype(np.uint8)) for c in labels] for z in range(B)]

    say(f"label volume: [{B}, {H}, {W}] uint8, labels {list(labels)}: {B * len(labels)} encodings")
    a, b = side_a(), side_b()
    c = side_c()
    t0 = time.perf_counter()
    c = side_c()
    tc = time.perf_counter() - t0
    same = all(torch.equal(x, y) and np.array_equal(x.cpu().numpy(), w) for ra, rb, rc in zip(a, b, c) for x, y, w in zip(ra, rb, rc))
    entries = sum(int(x.numel()) for row in a for x in row)
    say(f"  {entries} output entries; (a) == (b) == (c): {same}")
    del b, c
    t = alternate({"a": side_a, "b": side_b}, repeats, warmup=1)
    say(f"  (a) rle_encode_device          {fmt(t['a'])}   {vol.numel() / np.median(t['a']) / 1e9:8.2f} GB/s of mask bytes, end to end; one D2H read")
    say(f"  (b) torch-op chain on device   {fmt(t['b'])}   ({B * len(labels)} nonzero calls)")
    say(f"  (c) D2H + host rle_encode      {tc * 1e3:10.3f} ms (one run)")
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--edge", type=int, default=5000)
    ap.add_argument("--cube", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rle_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rle: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import rle as R

    dev = torch.device("cuda:0")
    say(f"run-length codec on {torch.cuda.get_device_name(dev)}; {args.repeats} alternating repeats (order reversed every round) after 2 warm-up runs of every side; "
        "host clock around device-synchronised calls")
    edge = args.edge
    labels_map = blob_labels((edge, edge), 4, 0, dev)
    g2 = torch.Generator().manual_seed(1)
    noise = (torch.rand((edge, edge), generator=g2) < 0.5).to(torch.uint8).to(dev)
    met1, ok1 = bench_2d("blob label map", labels_map, list(range(4)), args.repeats, R)
    met2, ok2 = bench_2d("50 % noise mask", noise, None, args.repeats, R)
    del labels_map, noise
    vol = blob_labels((args.cube,) * 3, 4, 2, dev)
    ok3 = bench_stack(vol, list(range(4)), max(3, args.repeats // 2), R)
    say(f"all outputs equal: {ok1 and ok2 and ok3}")
    say("THE BAR ((a) beats (b) by more than the spread on both 2-D inputs): " + ("met" if met1 and met2 else "NOT met"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
