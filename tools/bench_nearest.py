#!/usr/bin/env python3
"""Benchmark of the nearest-site kernels on one MI355X (utils/nearest.py, csrc/ptb_nearest.hip).

Inputs, seeded and generated here, those of tools/bench_distance.py: the 5000 x 5000 uint8 4-class blob label map, 50 % binary noise,
the 512^3 blob volume, a [64, 512, 512] stack of blob maps -- rows of nearest_site -- and, for expand_labels, the int32 cores
connected_components(distance_transform(blobs) > 6) of the blob map with the blob mask, made outside the timed region.

Timed, each call from its start to a device synchronise behind its last piece of work, after a warm-up of every side, in rounds that
alternate between the sides (the order inside a round turns over every round):
  (a) the new call                              -- nothing read back
  (h) the host route: D2H + scipy.ndimage.distance_transform_edt(return_distances=False, return_indices=True) + ravel_multi_index
      (the expansion row: + the fancy-index gather and the mask) + H2D; the stack entry by entry.  Without scipy on this machine the
      side is left out and the file says so.
  (d) distance_transform(squared=True) on the same map in the same process: (a) / (d) is the price of carrying the feature.  No bar
      is set on that ratio.
Reported per row: median and spread (max - min) of the repeats, and whether (a) and (h) agree: scipy breaks ties differently, so the
index maps are compared by the squared distance they imply, and the expansion by the share of positions that differ.
THE BAR: on the blob map, the noise map, the volume and the expansion row (a) beats (h) by more than the larger spread of the two.

Every row runs in a child process of its own under its own time limit; after a row that fails or runs out of time nothing more is
started.  --profile-map NAME runs the row's (a) and (d) three times each after one warm-up, for a per-kernel trace from outside.

    python tools/bench_nearest.py [--repeats 7] [--edge 5000] [--cube 512] [--out profiles/nearest_bench.txt]
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

ROWS = ("blobs", "noise", "volume", "stack", "expand")
BARRED = ("blobs", "noise", "volume", "expand")
ROW_LIMIT_S = {"blobs": 240, "noise": 240, "volume": 1100, "stack": 300, "expand": 300}


def host_index(h, dims, edt):
    """scipy's nearest site of every position of the numpy label map ``h`` (zeros are the sites), as int32 linear indices per entry"""
    stack = h.reshape((-1,) + h.shape[h.ndim - dims:])
    out = np.empty(stack.shape, np.int32)
    for e, o in zip(stack, out):
        idx = edt(e != 0, return_distances=False, return_indices=True)
        o[...] = np.ravel_multi_index(tuple(idx), e.shape)
    return out.reshape(h.shape)


def implied_squared(index, shape, dims):
    """int64 squared distance from every position to the site ``index`` names within its entry (device tensors)"""
    ent = shape[len(shape) - dims:]
    sq = torch.zeros(shape, dtype=torch.int64, device=index.device)
    rest = index.to(torch.int64)
    for k in range(dims - 1, -1, -1):
        n = ent[k]
        here = torch.arange(n, device=index.device).reshape((n,) + (1,) * (dims - 1 - k))
        sq += (rest % n - here) ** 2
        rest = rest // n
    return sq


def run_row(row, args):
    """one row in this process; prints its lines and a last line of JSON for the parent"""
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import connected_components, distance_transform, expand_labels, nearest_site

    dev = torch.device("cuda:0")
    labels, dims, _ = make_map("blobs" if row == "expand" else row, args.edge, args.cube, dev)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    if row == "expand":
        mask = labels != 0
        cores, count = connected_components(distance_transform(labels) > 6)
        subject = cores

        def side_a():
            return expand_labels(cores, mask=mask)

        def side_d():
            return distance_transform(cores, foreground=0, squared=True)

        def side_h(edt):
            c, m = cores.cpu().numpy(), mask.cpu().numpy()
            idx = edt(c == 0, return_distances=False, return_indices=True)
            return torch.from_numpy(np.where(m, c[tuple(idx)], 0)).to(dev)
        say(f"expand: {list(cores.shape)} int32 cores ({int(count)} components, {int((cores != 0).sum())} labelled positions) of the blob map, mask of {int(mask.sum())} positions")
    else:
        subject = labels

        def side_a():
            return nearest_site(labels, dims=dims)

        def side_d():
            return distance_transform(labels, dims=dims, squared=True)

        def side_h(edt):
            return torch.from_numpy(host_index(labels.cpu().numpy(), dims, edt)).to(dev)
        say(f"{row}: {list(labels.shape)} uint8, dims={dims}: {int((labels == 0).sum())} sites of {labels.numel()} positions")

    got = side_a()
    want_d = side_d()
    torch.cuda.synchronize()
    if row != "expand":
        same = bool((implied_squared(got, tuple(subject.shape), dims) == want_d).all())
        say(f"  (a) against (d): the returned sites lie at the squared distances of distance_transform: {'yes' if same else '**NO**'}")
    sides = {"a": side_a, "d": side_d}
    try:
        from scipy.ndimage import distance_transform_edt as edt

        sides["h"] = lambda: side_h(edt)
    except ImportError:
        say("  (h) left out: scipy is not installed on this machine")
    if "h" in sides:
        t0 = time.perf_counter()
        h = sides["h"]()                                      # (the host side's warm-up is also the result that is compared)
        say(f"  (h) first call {time.perf_counter() - t0:.1f} s")
        differ = int((h != got).sum())
        if row == "expand":
            say(f"  (a) against (h): {differ} of {got.numel()} positions differ (scipy breaks ties between equally near cores differently)")
        else:
            valid = bool((implied_squared(h, tuple(subject.shape), dims) == want_d).all())
            say(f"  (a) against (h): both name a site at the same exact distance: {'yes' if valid and same else '**NO**'}; {differ} of {got.numel()} indices differ "
                "(scipy breaks ties differently)")
        del h
    del got, want_d
    tm = alternate(sides, args.repeats)
    names = {"a": "expand_labels" if row == "expand" else "nearest_site", "h": "D2H + scipy return_indices + H2D", "d": "distance_transform(squared=True)"}
    for k, t in tm.items():
        say(f"  ({k}) {names[k]:42s} {fmt(t)}")
    say(f"  (a) / (d) = {np.median(tm['a']) / np.median(tm['d']):.2f}: the price of carrying the feature" + (" and of the gather" if row == "expand" else ""))
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
    from pytorch_toolbelt_amd.utils import connected_components, distance_transform, expand_labels, nearest_site

    dev = torch.device("cuda:0")
    labels, dims, _ = make_map("blobs" if row == "expand" else row, args.edge, args.cube, dev)
    if row == "expand":
        mask = labels != 0
        cores, _ = connected_components(distance_transform(labels) > 6)
    for _ in range(4):                       # (one warm-up and three calls; the per-kernel SHARES are what is read from the trace)
        if row == "expand":
            expand_labels(cores, mask=mask)
        else:
            nearest_site(labels, dims=dims)
            distance_transform(labels, dims=dims, squared=True)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--edge", type=int, default=5000)
    ap.add_argument("--cube", type=int, default=512)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", help="(internal) run one row in this process")
    ap.add_argument("--profile-map", choices=ROWS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_bench.txt"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("bench_nearest: at least 7 repeats")
    if not torch.cuda.is_available():
        sys.exit("bench_nearest: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    if args.profile_map:
        return profile_map(args.profile_map, args)
    if args.row:
        return run_row(args.row, args)
    lines = [f"nearest site and label expansion on {torch.cuda.get_device_name(0)}; {args.repeats} alternating repeats (order reversed every round) after 1 warm-up run "
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
    have = [r for r in BARRED if r in results]
    if failed or len(have) < len(BARRED):
        lines.append(f"THE BAR: **not established: of the rows {BARRED} only {tuple(have)} ran here**" + (f"; on those: {[(r, results[r]['bar']) for r in have]}" if have else ""))
    elif any(results[r]["bar"] is None for r in BARRED):
        lines.append("THE BAR: **not established: scipy is not installed on this machine**")
    else:
        lines.append("THE BAR ((a) beats the host route on the blob map, the noise map, the 512^3 volume and the expansion row by more than the spread): "
                     + ("met" if all(results[r]["bar"] for r in BARRED) else "**NOT met**") + f" {[(r, results[r]['bar']) for r in BARRED]}")
    print("\n".join(lines[-3:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
