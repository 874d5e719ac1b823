#!/usr/bin/env python3
"""Benchmark of the instance-matching kernels on one MI355X (utils/instances.py, csrc/ptb_instances.hip).

Rows, seeded and generated here, labelled with connected_components on the device (connectivity 8 / 26):
  blobs   a 5000 x 5000 pair of 4-class blob maps; the truth is the prediction shifted by (3, 5) with a corner cleared: most blobs match
  noise   a 5000 x 5000 pair of 50 % noise maps; the truth is the prediction with 5 % of its positions flipped
  volume  a 512^3 pair of 4-class blob volumes, perturbed like the blob maps

Timed, each call from its start to a device synchronise behind its last piece of work, after a warm-up of every side, in rounds that
alternate between the sides (the order inside a round turns over every round):
  (a) match_instances(thresholds=(0.5, 0.75, 0.9), num_pred=int, num_truth=int)   -- nothing read back
  (h) the host route: D2H of both int32 maps + the numpy recipe (np.unique of fused keys with counts, np.bincount areas, float64 IoU)
  (c) the torch-op chain on the device: torch.unique((p.long() << 32) | t.long(), return_counts=True), torch.bincount areas, IoU and the
      counts with torch ops
All three sides must agree on tp / fp / fn exactly.  Reported per row: median and spread (max - min) of the repeats, and the bytes a call
moves (a model: see bytes_moved) as a share of the copy rate measured in this process -- no claim is made about it: the workload is
latency- and atomic-bound.
THE BAR: on blobs and volume (a) beats (h) and (c) by more than the larger spread of the two sides.  The noise row is reported only.

Every row runs in a child process of its own under its own time limit; after a row that fails or runs out of time nothing more is
started.  --profile-row NAME runs match_instances twice on that row after one warm-up, for a per-kernel trace from outside.

    python tools/bench_instances.py [--repeats 7] [--edge 5000] [--cube 512] [--out profiles/instances_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_components import alternate, copy_rate, fmt  # noqa: E402

ROWS = ("blobs", "noise", "volume")
ROW_LIMIT_S = {"blobs": 300, "noise": 300, "volume": 600}
BAR_ROWS = ("blobs", "volume")
THRESHOLDS = (0.5, 0.75, 0.9)


def make_pair(row, edge, cube, dev):
    """(pred cc, truth cc, n_pred, n_truth) of a row, labelled on the device"""
    from bench_metrics import blob_labels
    from pytorch_toolbelt_amd.utils import connected_components

    if row == "noise":
        g = torch.Generator().manual_seed(1)
        a = torch.randint(0, 2, (edge, edge), generator=g, dtype=torch.uint8)
        b = torch.where(torch.rand((edge, edge), generator=g) < 0.05, 1 - a, a)
        a, b, dims, conn = a.to(dev), b.to(dev), 2, 8
    else:
        dims, conn = (2, 8) if row == "blobs" else (3, 26)
        a = blob_labels((edge, edge) if row == "blobs" else (cube,) * 3, 4, 0 if row == "blobs" else 2, dev)
        b = torch.roll(a, (3, 5), (-2, -1))
        b[(slice(0, max(1, a.shape[-1] // 12)),) * dims] = 0
    p, n_p = connected_components(a, connectivity=conn, dims=dims)
    t, n_t = connected_components(b, connectivity=conn, dims=dims)
    return p, t, int(n_p), int(n_t)


def counts_of(iou, present_p, present_t):
    tp = [int((iou > tau).sum()) for tau in THRESHOLDS]
    return [[v, present_p - v, present_t - v] for v in tp]


def host_route(p, t, n_p, n_t):
    hp, ht = p.cpu().numpy().reshape(-1).astype(np.int64), t.cpu().numpy().reshape(-1).astype(np.int64)
    area_p, area_t = np.bincount(hp, minlength=n_p + 1), np.bincount(ht, minlength=n_t + 1)
    both = (hp > 0) & (ht > 0)
    key, inter = np.unique((hp[both] << 32) | ht[both], return_counts=True)
    ip, it = key >> 32, key & 0xFFFFFFFF
    iou = inter.astype(np.float64) / (area_p[ip] + area_t[it] - inter).astype(np.float64)
    return counts_of(iou, int((area_p[1:] > 0).sum()), int((area_t[1:] > 0).sum()))


def chain(p, t, n_p, n_t):
    fp, ft = p.reshape(-1).long(), t.reshape(-1).long()
    area_p, area_t = torch.bincount(fp, minlength=n_p + 1), torch.bincount(ft, minlength=n_t + 1)
    both = (fp > 0) & (ft > 0)
    key, inter = torch.unique((fp[both] << 32) | ft[both], return_counts=True)
    ip, it = key >> 32, key & 0xFFFFFFFF
    iou = inter.double() / (area_p[ip] + area_t[it] - inter).double()
    return counts_of(iou, int((area_p[1:] > 0).sum()), int((area_t[1:] > 0).sum()))


def bytes_moved(n, n_p, n_t):
    """a model of the traffic of one match_instances call: both int32 maps read once; the table (16 bytes per slot, slots = the power of two
    >= 2 * min(n, n_p * n_t, 2^22)) set, and read by the match kernel; the per-instance outputs (24 bytes per instance) zeroed, written
    by the atomics or the match kernel and read by the count kernel"""
    slots = 2
    while slots < 2 * min(n, n_p * n_t, 1 << 22):
        slots *= 2
    return 8 * n + 2 * 16 * slots + 3 * 24 * (n_p + n_t)


def run_row(row, args):
    """one row in this process; prints its lines and a last line of JSON for the parent"""
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import match_instances

    dev = torch.device("cuda:0")
    p, t, n_p, n_t = make_pair(row, args.edge, args.cube, dev)
    rate = copy_rate(dev)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def side_a():
        return match_instances(p, t, THRESHOLDS, n_p, n_t)

    res = side_a()
    mine = [[int(res[k][j]) for k in ("tp", "fp", "fn")] for j in range(len(THRESHOLDS))]
    say(f"{row}: {list(p.shape)} int32 pair, {n_p} / {n_t} instances, {int(res['num_pairs'])} overlapping pairs; tp / fp / fn at {THRESHOLDS}: {mine}; "
        f"pq = {[round(float(v), 4) for v in res['pq']]}; copy rate here {rate / 1e12:.2f} TB/s")
    assert int(res["num_pairs"]) >= 0
    sides = {"a": side_a, "h": lambda: host_route(p, t, n_p, n_t), "c": lambda: chain(p, t, n_p, n_t)}
    agree = True
    for k in "hc":
        theirs = sides[k]()
        agree &= theirs == mine
        say(f"  ({k}) tp / fp / fn: {'equal' if theirs == mine else f'**DIFFERENT** {theirs}'}")
    tm = alternate(sides, args.repeats)
    names = {"a": "match_instances", "h": "D2H + numpy recipe", "c": "torch.unique chain on device"}
    for k, v in tm.items():
        extra = ""
        if k == "a":
            b = bytes_moved(p.numel(), n_p, n_t)
            extra = f"   {b / 1e6:8.0f} MB moved = {100 * b / np.median(v) / rate:5.1f} % of the copy rate"
        say(f"  ({k}) {names[k]:30s} {fmt(v)}{extra}")
    result = {"row": row, "agree": bool(agree), "bar": {}}
    for k in "hc":
        gap = float(np.median(tm[k]) - np.median(tm["a"]))
        spread = float(max(np.ptp(tm["a"]), np.ptp(tm[k])))
        met = gap > spread
        text = f"({k}) - (a) = {gap * 1e3:.3f} ms, larger spread {spread * 1e3:.3f} ms: {'ahead' if met else 'NOT ahead'} (({k}) / (a) = {np.median(tm[k]) / np.median(tm['a']):.1f})"
        say("  " + (text if met or row not in BAR_ROWS else f"**{text}**"))
        result["bar"][k] = met
    result["lines"] = lines
    print("RESULT " + json.dumps(result), flush=True)


def profile_row(row, args):
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import match_instances

    dev = torch.device("cuda:0")
    p, t, n_p, n_t = make_pair(row, args.edge, args.cube, dev)
    for _ in range(3):                       # (a warm-up and two calls; the per-kernel SHARES are what is read from the trace)
        match_instances(p, t, THRESHOLDS, n_p, n_t)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--edge", type=int, default=5000)
    ap.add_argument("--cube", type=int, default=512)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", help="(internal) run one row in this process")
    ap.add_argument("--profile-row", choices=ROWS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instances_bench.txt"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("bench_instances: at least 7 repeats")
    if not torch.cuda.is_available():
        sys.exit("bench_instances: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    if args.profile_row:
        return profile_row(args.profile_row, args)
    if args.row:
        return run_row(args.row, args)
    lines = [f"instance matching on {torch.cuda.get_device_name(0)}; {args.repeats} alternating repeats (order reversed every round) after 1 warm-up run "
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
    if failed or any(r not in results for r in BAR_ROWS):
        lines.append("THE BAR: **not established: a required row is missing**")
    else:
        met = all(results[r]["bar"][k] for r in BAR_ROWS for k in "hc") and all(r["agree"] for r in results.values())
        lines.append("THE BAR (match_instances beats the host route and the torch.unique chain on the blob maps and the volume by more than the spread, all "
                     "sides agreeing): " + ("met" if met else "**NOT met**") + f" {[(r, results[r]['bar']) for r in BAR_ROWS]}")
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
