#!/usr/bin/env python3
"""Benchmark of the watershed kernels on one MI355X (utils/watershed.py, csrc/ptb_watershed.hip).

Rows, seeded and generated here, outside the timed region:
  blobs    the 5000 x 5000 uint8 4-class blob map of tools/bench_distance.py: landscape -distance_transform(map), markers the int32 cores
           connected_components(distance_transform(map) > 6), mask map != 0 -- the documented recipe
  noise    a smoothed-noise float32 landscape of the same size (three 31-wide box filters over seeded normal noise), 2000 point seeds,
           no mask: long winding floods, the hard case for the sweep counts
  stack    a [64, 512, 512] stack of blob maps, the recipe of the first row
  volume   a 256^3 blob volume, dims=3, connectivity 26, cores at distance > 4

Timed, each call from its start to a device synchronise behind its last piece of work, after a warm-up of every side, in rounds that
alternate between the sides (the order inside a round turns over every round):
  (a) watershed(...)                            -- the call reads one word back per eight sweeps; both sweep counts are recorded
  (e) expand_labels on the same markers and mask in the same process: the device-side floor, since it answers an easier question
  (h) the host route a user has today: D2H + scipy.ndimage.watershed_ift on the landscape quantised to uint16 (markers -1 outside the
      mask) + H2D; the stack entry by entry.  A STAND-IN WITH A DIFFERENT ARC COST (|difference of heights|, not the pass height): it is
      timed only, never compared in value.  Without scipy on this machine the side is left out and the file says so.
THE BAR: on every row (a) beats (h) by more than the larger spread of the two.  A row that misses is printed in bold.

Every row runs in a child process of its own under its own time limit; after a row that fails or runs out of time nothing more is
started.  --profile-map NAME runs the row's (a) three times after one warm-up, for a per-kernel trace from outside.

    python tools/bench_watershed.py [--repeats 7] [--edge 5000] [--cube 256] [--out profiles/watershed_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_distance import alternate, fmt, make_map  # noqa: E402

ROWS = ("blobs", "noise", "stack", "volume")
ROW_LIMIT_S = {"blobs": 300, "noise": 300, "stack": 300, "volume": 300}


def make_row(row, edge, cube, dev):
    """``(height, markers, mask, dims, connectivity)`` on the device"""
    from pytorch_toolbelt_amd.utils import connected_components, distance_transform

    if row == "noise":
        g = torch.Generator().manual_seed(3)
        h = torch.randn((1, 1, edge, edge), generator=g).to(dev)
        for _ in range(3):
            h = torch.nn.functional.avg_pool2d(h, 31, stride=1, padding=15, count_include_pad=False)
        markers = torch.zeros(edge * edge, dtype=torch.int32)
        at = torch.randperm(edge * edge, generator=g)[:2000]
        markers[at] = torch.arange(1, 2001, dtype=torch.int32)
        return h.reshape(edge, edge).contiguous(), markers.reshape(edge, edge).to(dev), None, 2, 8
    labels, dims, _ = make_map(row, edge, cube, dev)
    d = distance_transform(labels, dims=dims)
    cores, _ = connected_components(d > (4 if dims == 3 else 6), dims=dims, connectivity=26 if dims == 3 else 8)
    return -d, cores, labels != 0, dims, 26 if dims == 3 else 8


def host_route(height, markers, mask, dims, ift):
    """D2H, scipy's image-foresting-transform watershed on a uint16 quantisation, H2D"""
    h, m = height.cpu().numpy(), markers.cpu().numpy().astype(np.int32)
    lo, hi = float(h.min()), float(h.max())
    q = np.round((h - lo) * (65535.0 / max(hi - lo, 1e-30))).astype(np.uint16)
    if mask is not None:
        m = np.where(mask.cpu().numpy(), m, -1)
    ent = lambda a: a.reshape((-1,) + a.shape[a.ndim - dims:])   # noqa: E731
    out = np.empty(m.shape, np.int32)
    for qe, me, oe in zip(ent(q), ent(m), ent(out)):
        oe[...] = np.maximum(ift(qe, me, structure=np.ones((3,) * dims, bool)), 0)
    return torch.from_numpy(out).to(height.device)


def run_row(row, args):
    """one row in this process; prints its lines and a last line of JSON for the parent"""
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import expand_labels, watershed

    dev = torch.device("cuda:0")
    height, markers, mask, dims, conn = make_row(row, args.edge, args.cube, dev)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def side_a():
        return watershed(height, markers, mask=mask, connectivity=conn, dims=dims)

    def side_e():
        return expand_labels(markers, mask=mask, dims=dims)

    got, sweeps = watershed(height, markers, mask=mask, connectivity=conn, dims=dims, return_sweeps=True)
    floor = side_e()
    torch.cuda.synchronize()
    say(f"{row}: {list(markers.shape)} {str(height.dtype)[6:]} landscape, dims={dims}, connectivity {conn}: {int((markers != 0).sum())} labelled positions, "
        f"{markers.numel() if mask is None else int(mask.sum())} flooded, {int((got != 0).sum())} reached; sweeps: cost {sweeps[0]}, path {sweeps[1]}")
    say(f"  (a) against (e): {int((got != floor).sum())} of {got.numel()} positions differ (the flood follows the landscape inside the mask, the expansion is Euclidean)")
    sides = {"a": side_a, "e": side_e}
    try:
        from scipy.ndimage import watershed_ift as ift

        sides["h"] = lambda: host_route(height, markers, mask, dims, ift)
    except ImportError:
        say("  (h) left out: scipy is not installed on this machine")
    if "h" in sides:
        t0 = time.perf_counter()
        sides["h"]()
        say(f"  (h) first call {time.perf_counter() - t0:.1f} s (a stand-in with a different arc cost: timed only, not compared in value)")
    del got, floor
    tm = alternate(sides, args.repeats)
    names = {"a": "watershed", "e": "expand_labels (the device-side floor)", "h": "D2H + scipy watershed_ift (uint16) + H2D"}
    for k, t in tm.items():
        say(f"  ({k}) {names[k]:42s} {fmt(t)}")
    say(f"  (a) / (e) = {np.median(tm['a']) / np.median(tm['e']):.2f}")
    result = {"row": row, "median_a": float(np.median(tm["a"])), "sweeps": list(sweeps), "bar": None}
    if "h" in tm:
        gap = float(np.median(tm["h"]) - np.median(tm["a"]))
        spread = float(max(np.ptp(tm["a"]), np.ptp(tm["h"])))
        met = gap > spread
        text = f"(h) - (a) = {gap * 1e3:.3f} ms, larger spread {spread * 1e3:.3f} ms: (a) {'beats' if met else 'does NOT beat'} (h) by more than the spread ((h) / (a) = {np.median(tm['h']) / np.median(tm['a']):.1f})"
        say("  " + (text if met else f"**{text}**"))
        result["bar"] = met
    result["lines"] = lines
    print("RESULT " + json.dumps(result), flush=True)


def profile_map(row, args):
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import watershed

    dev = torch.device("cuda:0")
    height, markers, mask, dims, conn = make_row(row, args.edge, args.cube, dev)
    for _ in range(4):                       # (one warm-up and three calls; the per-kernel SHARES are what is read from the trace)
        watershed(height, markers, mask=mask, connectivity=conn, dims=dims)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--edge", type=int, default=5000)
    ap.add_argument("--cube", type=int, default=256)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", help="(internal) run one row in this process")
    ap.add_argument("--profile-map", choices=ROWS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "watershed_bench.txt"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("bench_watershed: at least 7 repeats")
    if not torch.cuda.is_available():
        sys.exit("bench_watershed: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    if args.profile_map:
        return profile_map(args.profile_map, args)
    if args.row:
        return run_row(args.row, args)
    lines = [f"marker-controlled watershed on {torch.cuda.get_device_name(0)}; {args.repeats} alternating repeats (order reversed every round) after 1 warm-up run "
             "of every side; host clock around device-synchronised calls; every row in a process of its own under its own time limit"]
    print(lines[0], flush=True)
    results, failed = {}, None
    for row in args.rows.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--repeats", str(args.repeats), "--edge", str(args.edge), "--cube", str(args.cube)]
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
        if timed_out:
            failed = f"{row}: no result within its time limit of {ROW_LIMIT_S[row]} s; nothing more was started"
            break
        res = [ln for ln in stdout if ln.startswith("RESULT ")]
        if child.returncode != 0 or not res:
            failed = f"{row}: exit status {child.returncode}; nothing more was started\n" + stderr[-2000:]
            break
        results[row] = json.loads(res[-1][7:])
        lines += results[row]["lines"]
    if failed:
        lines.append("**" + failed + "**")
    have = [r for r in ROWS if r in results]
    if failed or len(have) < len(ROWS):
        lines.append(f"THE BAR: **not established: of the rows {ROWS} only {tuple(have)} ran here**" + (f"; on those: {[(r, results[r]['bar']) for r in have]}" if have else ""))
    elif any(results[r]["bar"] is None for r in ROWS):
        lines.append("THE BAR: **not established: scipy is not installed on this machine**")
    else:
        lines.append("THE BAR ((a) beats the host route on every row by more than the spread): "
                     + ("met" if all(results[r]["bar"] for r in ROWS) else "**NOT met**") + f" {[(r, results[r]['bar']) for r in ROWS]}")
    print("\n".join(lines[-3:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
