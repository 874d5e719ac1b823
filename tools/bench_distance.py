#!/usr/bin/env python3
"""Benchmark of the distance-transform kernels on one MI355X (utils/distance.py, csrc/ptb_distance.hip).

Inputs, seeded and generated here.  5000 x 5000 uint8: a 4-class blob label map as merge_crop(argmax=True, dtype=torch.uint8) leaves
it, 50 % binary noise, all object with a single site (one parabola per line, the longest distances), no site at all (inf everywhere),
and the blob map again with signed=True.  A [64, 512, 512] stack of blob maps.  512^3: a 4-class blob volume with unit spacing and
with spacing (2.5, 0.7, 0.7).

Timed, each call from its start to a device synchronise behind its last piece of work, after a warm-up of every side, in rounds that
alternate between the sides (the order inside a round turns over every round):
  (a) distance_transform                        -- nothing read back
  (h) the host route: D2H + scipy.ndimage.distance_transform_edt + H2D of the float32 result (signed: two transforms and their
      difference; the stack: entry by entry, as scipy has no batch axis).  Without scipy on this machine the side is left out and the
      file says so.  There is no honest torch-op chain for this operation, so none is claimed.
Reported per row: median and spread (max - min) of the repeats, the modelled bytes of a call (see bytes_moved) against the copy rate
measured in this process -- nothing is claimed as a share of peak: the line passes are latency-bound -- and whether the sides agree
(entries without a site, where scipy measures to a virtual site at index -1 and this library returns inf, are left out of that).
THE BAR: on the blob map, on the noise map and on the 512^3 volume with unit spacing (a) beats (h) by more than the larger spread
of the two.  The remaining rows are reported only.

Every row runs in a child process of its own under its own time limit; after a row that fails or runs out of time nothing more is
started.  --profile-map NAME runs distance_transform twice on that map after one warm-up, for a per-kernel trace from outside.

    python tools/bench_distance.py [--repeats 7] [--edge 5000] [--cube 512] [--out profiles/distance_bench.txt]
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

ROWS = ("blobs", "noise", "one_site", "no_site", "blobs_signed", "stack", "volume", "volume_spacing")
BARRED = ("blobs", "noise", "volume")
ROW_LIMIT_S = {"blobs": 240, "noise": 240, "one_site": 240, "no_site": 240, "blobs_signed": 300, "stack": 300, "volume": 1100, "volume_spacing": 1100}
SPACING = (2.5, 0.7, 0.7)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def alternate(sides, repeats):
    """(the warm-up of every side is the call whose result run_row compares)"""
    times = {k: [] for k in sides}
    order = list(sides)
    for r in range(repeats):
        for k in (order if r % 2 == 0 else order[::-1]):
            times[k].append(once(sides[k]))
    return {k: np.array(v) for k, v in times.items()}


def make_map(row, edge, cube, dev):
    """(labels, dims, keyword arguments of the call)"""
    from bench_metrics import blob_labels

    if row in ("blobs", "blobs_signed"):
        return blob_labels((edge, edge), 4, 0, dev), 2, dict(signed=row == "blobs_signed")
    if row == "noise":
        g = torch.Generator().manual_seed(1)
        return torch.randint(0, 2, (edge, edge), generator=g, dtype=torch.uint8).to(dev), 2, {}
    if row == "one_site":
        a = torch.ones((edge, edge), dtype=torch.uint8, device=dev)
        a[edge // 3, edge // 7] = 0
        return a, 2, {}
    if row == "no_site":
        return torch.ones((edge, edge), dtype=torch.uint8, device=dev), 2, {}
    if row == "stack":
        return torch.stack([blob_labels((512, 512), 4, 10 + k, dev) for k in range(64)]), 2, {}
    return blob_labels((cube,) * 3, 4, 2, dev), 3, dict(spacing=SPACING) if row == "volume_spacing" else {}


def copy_rate(dev):
    """bytes per second (read + written) of a 256 MB device-to-device copy, the median of 5"""
    src = torch.empty(64 << 20, dtype=torch.int32, device=dev)
    dst = torch.empty_like(src)
    once(lambda: dst.copy_(src))
    t = np.median([once(lambda: dst.copy_(src)) for _ in range(5)])
    return 2 * src.numel() * 4 / t


def bytes_moved(n, elem, dims, signed):
    """a model of the traffic of one call over n positions: the row pass reads the map and writes, reads and writes its 32-bit map; every
    line pass reads one 32-bit map and writes one.  The envelope's stack traffic (8 bytes per push and per pop, which depends on the
    map) and the gathers of g at popped vertices are left out.  signed: everything twice, plus the read of the first run's result."""
    run = n * (elem + 12 + 8 * (dims - 1))
    return run if not signed else 2 * run + 4 * n


def host_route(labels, dims, edt, dev, spacing=None, signed=False):
    h = labels.cpu().numpy()
    out = np.empty(h.shape, np.float32)
    stack = h.reshape((-1,) + h.shape[h.ndim - dims:])
    for e, o in zip(stack, out.reshape(stack.shape)):
        d = edt(e != 0, sampling=spacing)
        if signed:
            d = edt(e == 0, sampling=spacing) - d
        o[...] = d
    return torch.from_numpy(out).to(dev)


def fmt(t):
    return f"{np.median(t) * 1e3:10.3f} ms (spread {(t.max() - t.min()) * 1e3:8.3f} ms)"


def run_row(row, args):
    """one row in this process; prints its lines and a last line of JSON for the parent"""
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import distance_transform

    dev = torch.device("cuda:0")
    labels, dims, kw = make_map(row, args.edge, args.cube, dev)
    rate = copy_rate(dev)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def side_a():
        return distance_transform(labels, dims=dims, **kw)

    d = side_a()
    torch.cuda.synchronize()
    n = labels.numel()
    finite = torch.isfinite(d)
    largest = float(d[finite].abs().max()) if bool(finite.any()) else float("inf")
    say(f"{row}: {list(labels.shape)} uint8, dims={dims}{''.join(f', {k}={v}' for k, v in kw.items() if v)}: {int((labels == 0).sum())} sites of {n} positions, "
        f"largest finite |distance| {largest:.2f}, {int((~finite).sum())} positions without a site; copy rate here {rate / 1e12:.2f} TB/s")
    sides = {"a": side_a}
    try:
        from scipy.ndimage import distance_transform_edt as edt

        sides["h"] = lambda: host_route(labels, dims, edt, dev, spacing=kw.get("spacing"), signed=kw.get("signed", False))
    except ImportError:
        say("  (h) left out: scipy is not installed on this machine")
    if "h" in sides:
        t0 = time.perf_counter()
        h = sides["h"]()                                      # (the host side's warm-up is also the result that is compared)
        say(f"  (h) first call {time.perf_counter() - t0:.1f} s")
        if bool(finite.all()):
            rel = float(((d - h).abs() / h.abs().clamp_min(1e-30)).max())
            say(f"  (a) against (h): largest relative difference {rel:.2e}: {'equal within 1e-6' if rel <= 1e-6 else '**DIFFERENT**'}")
        else:
            say(f"  (a) against (h): not compared, the map has no site ((h) measures to a virtual site at index -1 and is finite: {bool(torch.isfinite(h).all())})")
        del h
    del d, finite
    tm = alternate(sides, args.repeats)
    names = {"a": "distance_transform", "h": "D2H + scipy distance_transform_edt + H2D"}
    for k, t in tm.items():
        extra = ""
        if k == "a":
            b = bytes_moved(n, 1, dims, kw.get("signed", False))
            extra = f"   {b / 1e6:8.0f} MB modelled = {100 * b / np.median(t) / rate:5.1f} % of the copy rate"
        say(f"  ({k}) {names[k]:42s} {fmt(t)}{extra}")
    result = {"row": row, "median_a": float(np.median(tm["a"])), "bar": None}
    if "h" in tm:
        gap = float(np.median(tm["h"]) - np.median(tm["a"]))
        spread = float(max(np.ptp(tm["a"]), np.ptp(tm["h"])))
        met = gap > spread
        text = f"(h) - (a) = {gap * 1e3:.3f} ms, larger spread {spread * 1e3:.3f} ms: (a) {'beats' if met else 'does NOT beat'} (h) by more than the spread ((h) / (a) = {np.median(tm['h']) / np.median(tm['a']):.1f})"
        say("  " + (text if met or row not in BARRED else f"**{text}**") + ("" if row in BARRED else "   [reported, not barred]"))
        if row in BARRED:
            result["bar"] = met
    result["lines"] = lines
    print("RESULT " + json.dumps(result), flush=True)


def profile_map(row, args):
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import distance_transform

    dev = torch.device("cuda:0")
    labels, dims, kw = make_map(row, args.edge, args.cube, dev)
    for _ in range(3):                       # (the trace holds all three; the per-kernel SHARES are what is read from it)
        distance_transform(labels, dims=dims, **kw)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--edge", type=int, default=5000)
    ap.add_argument("--cube", type=int, default=512)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", help="(internal) run one row in this process")
    ap.add_argument("--profile-map", choices=ROWS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_bench.txt"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("bench_distance: at least 7 repeats")
    if not torch.cuda.is_available():
        sys.exit("bench_distance: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    if args.profile_map:
        return profile_map(args.profile_map, args)
    if args.row:
        return run_row(args.row, args)
    lines = [f"distance transform on {torch.cuda.get_device_name(0)}; {args.repeats} alternating repeats (order reversed every round) after 1 warm-up run "
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
    if "blobs" in results:
        for k in ("one_site", "no_site", "blobs_signed"):
            if k in results:
                lines.append(f"{k} / blobs, (a): {results[k]['median_a'] / results['blobs']['median_a']:.2f}")
    have = [r for r in BARRED if r in results]
    if failed or len(have) < len(BARRED):
        lines.append(f"THE BAR: **not established: of the rows {BARRED} only {tuple(have)} ran here**" + (f"; on those: {[(r, results[r]['bar']) for r in have]}" if have else ""))
    elif any(results[r]["bar"] is None for r in BARRED):
        lines.append("THE BAR: **not established: scipy is not installed on this machine**")
    else:
        lines.append("THE BAR ((a) beats the host route on the blob map, the noise map and the 512^3 volume by more than the spread): "
                     + ("met" if all(results[r]["bar"] for r in BARRED) else "**NOT met**") + f" {[(r, results[r]['bar']) for r in BARRED]}")
    print("\n".join(lines[-5:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
