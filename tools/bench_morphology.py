#!/usr/bin/env python3
"""Benchmark of the morphology kernels on one MI355X (utils/morphology.py, csrc/ptb_morphology.hip).

Rows, seeded and generated here, outside the timed region:
  u8_disk3     opening of an --edge x --edge uint8 map (the blob map of tools/bench_distance.py scaled to 0 .. 255, plus noise) with disk(3)
  f32_disk15   opening of the same map as float32 with disk(15)
  blobs_disk5  binary_opening of the 4-class blob map (everything that is not class 0) with disk(5), border_value=None
  stack        binary_opening of a [64, 512, 512] stack of blob maps with disk(5), border_value=None

Timed, each call from its start to a device synchronise behind its last piece of work, after a warm-up of every side (the call whose
result is compared), in rounds that alternate between the sides (the order turns over every round):
  (a) the device call
  (h) D2H + scipy.ndimage (grey_opening / binary_opening with the matching border) + H2D; compared with (a) bit for bit
  (c) the best composition available on the device without these kernels: grey rows, a chain of torch.minimum / maximum over shifted
      slices of a padded copy, one pair of ops per footprint offset; binary rows, two distance_transform calls and two thresholds
      (squared distance > r^2, then <= r^2 to what is left); compared with (a) bit for bit
THE BAR: on every row (a) beats (h) and (c) by more than the larger spread of the two sides.  A row that misses is printed in bold.
--host-repeats N times (h) N times only (at least 3), each next to a device call of the same round; the file says so.

Every row runs in a child process of its own under its own time limit; after a row that fails or runs out of time nothing more is
started.  The file is rewritten after every row.

    python tools/bench_morphology.py [--repeats 7] [--host-repeats 3] [--edge 5000] [--out profiles/morphology_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import threading

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_distance import fmt, make_map, once  # noqa: E402

ROWS = {"u8_disk3": 3, "f32_disk15": 15, "blobs_disk5": 5, "stack": 5}         # row -> the disk's radius
ROW_LIMIT_S = {"u8_disk3": 600, "f32_disk15": 1500, "blobs_disk5": 600, "stack": 600}


def chain_grey(x, off, dilate):
    """E or D of ``x`` [H, W] with torch ops: the minimum (maximum) over shifted slices of a copy padded with the identity"""
    H, W = x.shape
    r = int(np.abs(off).max())
    top = float("inf") if x.dtype.is_floating_point else torch.iinfo(x.dtype).max
    low = float("-inf") if x.dtype.is_floating_point else torch.iinfo(x.dtype).min
    p = F.pad(x, (r, r, r, r), value=low if dilate else top)
    acc = None
    for dy, dx in (-off if dilate else off):
        v = p[r + dy:r + dy + H, r + dx:r + dx + W]
        acc = v if acc is None else (torch.maximum(acc, v) if dilate else torch.minimum(acc, v))
    return acc


def run_row(row, args):
    """one row in this process; prints its lines and a last line of JSON for the parent"""
    import scipy.ndimage as ndi

    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import binary_opening, disk, distance_transform, opening

    dev = torch.device("cuda:0")
    radius = ROWS[row]
    fp = disk(radius)
    off = np.argwhere(fp) - radius
    binary = row in ("blobs_disk5", "stack")
    labels = make_map("stack" if row == "stack" else "blobs", args.edge, 0, dev)[0]
    if binary:
        x = labels

        def side_a():
            return binary_opening(x, fp, border_value=None)

        def side_h():
            m = (x != 0).cpu().numpy().reshape((-1,) + x.shape[-2:])
            res = np.stack([ndi.binary_dilation(ndi.binary_erosion(p, structure=fp, border_value=1), structure=fp, border_value=0) for p in m])
            return torch.from_numpy(res.reshape(x.shape)).to(dev)

        def side_c():
            kept = distance_transform(x, squared=True) > radius * radius
            return distance_transform(kept.to(torch.uint8), background=1, squared=True) <= radius * radius       # (the sites: what was kept)
    else:
        gen = torch.Generator().manual_seed(3)
        x = (labels.to(torch.int32) * 60 + torch.randint(0, 76, labels.shape, generator=gen).to(dev)).to(torch.uint8)
        if row == "f32_disk15":
            x = x.to(torch.float32) / 4

        def side_a():
            return opening(x, fp)

        def side_h():
            a = x.cpu().numpy()
            e = ndi.grey_erosion(a, footprint=fp, mode="constant", cval=np.inf if a.dtype.kind == "f" else 255)
            return torch.from_numpy(ndi.grey_dilation(e, footprint=fp, mode="constant", cval=-np.inf if a.dtype.kind == "f" else 0)).to(dev)

        def side_c():
            return chain_grey(chain_grey(x, off, False), off, True)

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    fns = {"a": side_a, "h": side_h, "c": side_c}
    got = side_a()
    same = {k: bool(torch.equal(fns[k](), got)) for k in ("h", "c")}           # (the warm-up of the two other sides)
    say(f"{row}: {list(x.shape)} {x.dtype}, disk({radius}) = {int(fp.sum())} offsets in {fp.shape[0]} runs: {'binary_opening' if binary else 'opening'}")
    say("  " + "; ".join(f"(a) {'equals' if ok else '**DIFFERS FROM**'} ({k}) bit for bit" for k, ok in same.items()))
    once(side_a)
    times = {k: [] for k in fns}
    for r in range(args.repeats):
        for k in (("a", "h", "c") if r % 2 == 0 else ("c", "h", "a")):
            if k == "h" and r >= args.host_repeats:
                continue
            times[k].append(once(fns[k]))
    tm = {k: np.array(v) for k, v in times.items()}
    names = {"a": "the device call", "h": "D2H + scipy.ndimage + H2D", "c": "the composition of what the device had before"}
    for k in fns:
        say(f"  ({k}) {names[k]:48s} {fmt(tm[k])}  [{len(tm[k])} samples]")
    met = all(same.values())
    for k in ("h", "c"):
        gap, spread = float(np.median(tm[k]) - np.median(tm["a"])), float(max(np.ptp(tm["a"]), np.ptp(tm[k])))
        ok = gap > spread
        met = met and ok
        text = (f"({k}) - (a) = {gap * 1e3:.3f} ms, larger spread {spread * 1e3:.3f} ms: (a) {'beats' if ok else 'does NOT beat'} ({k}) by more than the spread "
                f"(({k}) / (a) = {np.median(tm[k]) / np.median(tm['a']):.1f})")
        say("  " + (text if ok else f"**{text}**"))
    print("RESULT " + json.dumps({"row": row, "bar": met, "lines": lines}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=None)
    ap.add_argument("--edge", type=int, default=5000)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", help="(internal) run one row in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morphology_bench.txt"))
    args = ap.parse_args()
    if args.host_repeats is None:
        args.host_repeats = args.repeats
    if args.repeats < 7 or not 3 <= args.host_repeats <= args.repeats:
        sys.exit("bench_morphology: at least 7 repeats and between 3 and --repeats host repeats")
    if not torch.cuda.is_available():
        sys.exit("bench_morphology: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    if args.row:
        return run_row(args.row, args)
    lines = [f"opening and binary_opening on {torch.cuda.get_device_name(0)}, edge {args.edge}; {args.repeats} alternating repeats (order reversed every round; the host side (h) "
             f"in {args.host_repeats} of them) after 1 warm-up run of every side; host clock around device-synchronised calls; every row in a process of its own under its own time limit"]
    print(lines[0], flush=True)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")

    bars, failed = {}, None
    for row in args.rows.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--repeats", str(args.repeats), "--host-repeats", str(args.host_repeats), "--edge", str(args.edge)]
        child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        timed_out = []
        timer = threading.Timer(ROW_LIMIT_S[row], lambda: (timed_out.append(True), child.kill()))
        timer.start()
        stdout = []
        for ln in child.stdout:                       # (echoed as it comes: a long row is not a silent one)
            stdout.append(ln.rstrip("\n"))
            if not ln.startswith("RESULT "):
                print(ln, end="", flush=True)
        stderr = child.stderr.read()
        child.wait()
        timer.cancel()
        res = [ln for ln in stdout if ln.startswith("RESULT ")]
        if timed_out or child.returncode != 0 or not res:
            failed = (f"{row}: no result within its time limit of {ROW_LIMIT_S[row]} s" if timed_out else f"{row}: exit status {child.returncode}\n" + stderr[-2000:]) + "; nothing more was started"
            break
        r = json.loads(res[-1][7:])
        bars[row] = r["bar"]
        lines += r["lines"]
        write()
    if failed:
        lines.append("**" + failed + "**")
    lines.append("THE BAR ((a) beats (h) and (c) on every row by more than the spread): "
                 + ("met" if not failed and len(bars) == len(ROWS) and all(bars.values()) else f"**NOT met or not established**") + f" {sorted(bars.items())}")
    print(lines[-1], flush=True)
    write()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
