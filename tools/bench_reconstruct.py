#!/usr/bin/env python3
"""Benchmark of the reconstruction kernels on one MI355X (utils/reconstruct.py, csrc/ptb_reconstruct.hip).

Rows, seeded and generated here, outside the timed region (the maps of tools/bench_distance.py):
  fill     (a) the 5000 x 5000 uint8 4-class blob map as a bool mask: fill_holes(sem)
  hmax     (b) the same map: h_maxima(distance_transform(sem), 2.0, domain=sem != 0); the distance map is computed outside the timed region
  stack    (c) a [64, 512, 512] stack of blob maps, the call of (b)
  volume   (d) a 256^3 blob volume, dims=3, connectivity 26, the call of (b)

Timed, each call from its start to a device synchronise behind its last piece of work, after a warm-up of every side, in rounds that
alternate between the sides (the order inside a round turns over every round):
  (a) the device call -- it reads one word back per eight sweeps; the sweep counts of its phases are recorded
  (h) the host route a user has today: fill: D2H + scipy.ndimage.binary_fill_holes + H2D.  hmax / stack / volume: D2H + THE LIBRARY'S OWN
      CPU FORM + H2D -- A STAND-IN, because scikit-image is not installed where this runs; its result is compared with (a), bit for bit
  (t) hmax only, without a bar: the threshold recipe connected_components(distance_transform(sem) > r) on the same map, distance
      transform included, next to (c2) = distance_transform + h_maxima + connected_components
THE BAR: on every row (a) beats (h) by more than the larger spread of the two.  A row that misses is printed in bold.
--host-repeats N times the host side N times only (at least 3), each next to a device call of the same round; the file says so.

Every row runs in a child process of its own under its own time limit; after a row that fails or runs out of time nothing more is
started.  --profile-map NAME runs the row's (a) three times after one warm-up, for a per-kernel trace from outside.

    python tools/bench_reconstruct.py [--repeats 7] [--edge 5000] [--cube 256] [--out profiles/reconstruct_bench.txt]
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

from bench_distance import fmt, make_map, once  # noqa: E402

ROWS = ("fill", "hmax", "stack", "volume")
MAPS = {"fill": "blobs", "hmax": "blobs", "stack": "stack", "volume": "volume"}
ROW_LIMIT_S = {"fill": 400, "hmax": 900, "stack": 900, "volume": 900}
H = 2.0


def make_row(row, edge, cube, dev):
    """``(sem bool, distance map or None, dims, connectivity)`` on the device"""
    from pytorch_toolbelt_amd.utils import distance_transform

    labels, dims, _ = make_map(MAPS[row], edge, cube, dev)
    sem = labels != 0
    if row == "fill":
        return sem, None, dims, None
    return sem, distance_transform(labels, dims=dims), dims, 26 if dims == 3 else 8


def run_row(row, args):
    """one row in this process; prints its lines and a last line of JSON for the parent"""
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import connected_components, distance_transform, fill_holes, h_maxima

    dev = torch.device("cuda:0")
    sem, d, dims, conn = make_row(row, args.edge, args.cube, dev)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    if row == "fill":
        from scipy.ndimage import binary_fill_holes

        def side_a():
            return fill_holes(sem)

        def side_h():
            return torch.from_numpy(binary_fill_holes(sem.cpu().numpy())).to(dev)

        got, sweeps = fill_holes(sem, return_sweeps=True)
        what_h = "D2H + scipy binary_fill_holes + H2D"
    else:
        def side_a():
            return h_maxima(d, H, connectivity=conn, domain=sem, dims=dims)

        def side_h():
            return h_maxima(d.cpu(), H, connectivity=conn, domain=sem.cpu(), dims=dims).to(dev)

        got, sweeps = h_maxima(d, H, connectivity=conn, domain=sem, dims=dims, return_sweeps=True)
        what_h = "D2H + the library's CPU form + H2D (STAND-IN)"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = side_h()
    first = time.perf_counter() - t0
    same = bool(torch.equal(ref, got))
    say(f"{row}: {list(sem.shape)} dims={dims}{'' if conn is None else f', connectivity {conn}, h = {H}'}: {int(sem.sum())} of {sem.numel()} positions set, "
        f"{int((got != sem).sum()) if row == 'fill' else int(got.sum())} {'filled' if row == 'fill' else 'positions in extended maxima'}; sweeps: {sweeps[0]}"
        + (f" and {sweeps[1]}" if row != "fill" else ""))
    say(f"  (h) first call {first:.1f} s; (a) {'equals' if same else '**DIFFERS FROM**'} (h) bit for bit")
    del ref, got
    times = {"a": [], "h": []}
    for r in range(args.repeats):
        both = r < args.host_repeats
        for k in (("a", "h") if r % 2 == 0 else ("h", "a")):
            if k == "a" or both:
                times[k].append(once(side_a if k == "a" else side_h))
    tm = {k: np.array(v) for k, v in times.items()}
    say(f"  (a) {'fill_holes' if row == 'fill' else 'h_maxima':46s} {fmt(tm['a'])}")
    say(f"  (h) {what_h:46s} {fmt(tm['h'])}" + ("" if args.host_repeats >= args.repeats else f"  [{args.host_repeats} repeats]"))
    gap = float(np.median(tm["h"]) - np.median(tm["a"]))
    spread = float(max(np.ptp(tm["a"]), np.ptp(tm["h"])))
    met = gap > spread and same
    text = f"(h) - (a) = {gap * 1e3:.3f} ms, larger spread {spread * 1e3:.3f} ms: (a) {'beats' if met else 'does NOT beat'} (h) by more than the spread ((h) / (a) = {np.median(tm['h']) / np.median(tm['a']):.1f})"
    say("  " + (text if met else f"**{text}**"))
    if row == "hmax":                                  # without a bar: the two seed recipes end to end, and the plain-domain call
        labels = make_map("blobs", args.edge, args.cube, dev)[0]

        def chain():
            dd = distance_transform(labels)
            return connected_components(h_maxima(dd, H, domain=labels != 0))

        def threshold():
            return connected_components(distance_transform(labels) > 6)

        n_c, n_t = int(chain()[1]), int(threshold()[1])
        tc = np.array([once(chain) for _ in range(args.repeats)])
        tt = np.array([once(threshold) for _ in range(args.repeats)])
        say(f"  (c2) distance_transform + h_maxima + connected_components: {n_c} cores {fmt(tc)}")
        say(f"  (t)  distance_transform > 6 + connected_components:         {n_t} cores {fmt(tt)}")
        _, free = h_maxima(d, H, connectivity=conn, return_sweeps=True)
        tf = np.array([once(lambda: h_maxima(d, H, connectivity=conn)) for _ in range(args.repeats)])
        say(f"  (n)  h_maxima without domain= (the background is one plateau): sweeps {free[0]} and {free[1]} {fmt(tf)}")
    result = {"row": row, "median_a": float(np.median(tm["a"])), "sweeps": list(sweeps), "bar": bool(met), "lines": lines}
    print("RESULT " + json.dumps(result), flush=True)


def profile_map(row, args):
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import fill_holes, h_maxima

    dev = torch.device("cuda:0")
    sem, d, dims, conn = make_row(row, args.edge, args.cube, dev)
    for _ in range(4):                       # (one warm-up and three calls; the per-kernel SHARES are what is read from the trace)
        if row == "fill":
            fill_holes(sem)
        else:
            h_maxima(d, H, connectivity=conn, domain=sem, dims=dims)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=None)
    ap.add_argument("--edge", type=int, default=5000)
    ap.add_argument("--cube", type=int, default=256)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", help="(internal) run one row in this process")
    ap.add_argument("--profile-map", choices=ROWS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruct_bench.txt"))
    args = ap.parse_args()
    if args.host_repeats is None:
        args.host_repeats = args.repeats
    if args.repeats < 7 or not 3 <= args.host_repeats <= args.repeats:
        sys.exit("bench_reconstruct: at least 7 repeats, and between 3 and --repeats host repeats")
    if not torch.cuda.is_available():
        sys.exit("bench_reconstruct: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    if args.profile_map:
        return profile_map(args.profile_map, args)
    if args.row:
        return run_row(args.row, args)
    lines = [f"reconstruction, h-maxima and hole filling on {torch.cuda.get_device_name(0)}; {args.repeats} alternating repeats (order reversed every round; the host side in "
             f"{args.host_repeats} of them) after 1 warm-up run of every side; host clock around device-synchronised calls; every row in a process of its own under its own time limit"]
    print(lines[0], flush=True)
    results, failed = {}, None
    rows = args.rows.split(",")
    for row in rows:
        cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--repeats", str(args.repeats), "--host-repeats", str(args.host_repeats), "--edge", str(args.edge),
               "--cube", str(args.cube)]
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
