#!/usr/bin/env python3
"""Benchmark of the skeleton kernels on one MI355X (utils/skeleton.py, csrc/ptb_skeleton.hip).

Rows, seeded and generated here, outside the timed region (the maps of tools/bench_distance.py):
  blobs    the --edge x --edge uint8 4-class blob map: skeletonize(labels), everything that is not class 0
  noise    50 % noise of that size                                     (reported without a bar)
  ones     all ones of that size, the deepest case: edge / 2 iterations (reported without a bar; (h) is not run: it would take hours)
  stack    a [64, 512, 512] stack of blob maps
  cldice   centerline_dice of the blob map and the same map shifted by (3, 5), labels 0 .. 3

Timed, each call from its start to a device synchronise behind its last piece of work, after a warm-up of every side, in rounds that
alternate between the sides (the order inside a round turns over every round):
  (a) the device call; its iteration count is recorded
  (h) D2H + THE LIBRARY'S OWN CPU FORM + H2D -- A STAND-IN for the host route, because neither scikit-image nor OpenCV is installed where
      this runs; its result is compared with (a), bit for bit
  (c) the same formulae as a chain of torch ops on the device: shifted slices of a padded bool tensor, .any() per iteration
THE BAR: on blobs, stack and cldice (a) beats (h) and (c) by more than the larger spread of the two sides.  A row that misses is printed in bold.
--host-repeats N times (h) N times only (at least 3), each next to a device call of the same round; the file says so.  The CPU form of
the cldice row thins eight maps and takes minutes per call: --cldice-host-repeats N (default: --host-repeats) sets its samples apart;
with 0 its one compared call is its only sample, the row says so, and the (h) half of its bar is then stated as NOT established.

Every row runs in a child process of its own under its own time limit (sized for the default invocation: 8 calls of (h)); after a row
that fails or runs out of time nothing more is started.  The file is rewritten after every row.

    python tools/bench_skeleton.py [--repeats 7] [--edge 5000] [--out profiles/skeleton_bench.txt]

TWO SECTIONS OF THE FILE ARE NOT MEASURED BY A PLAIN RUN and are kept by it: everything from the line that starts with KEPT_MARKER on is
copied from the existing file into the new one.
  The STEPS comparison: build the library with another step count into a directory of its own,
      python -c "import __graft_entry__ as g; g.FLAGS.append('-DPTB_THIN_STEPS=8'); g.build(force=True, out_dir='build/steps8')"
  (and 16, 32), then  PTB_HIP_LIB=build/steps8/libptb_hip.so python tools/bench_skeleton.py --steps-row  prints that library's line.
  The kernel-time split: --profile-row NAME runs the row's (a) three times after one warm-up, for
      rocprofv3 --kernel-trace --stats -- python tools/bench_skeleton.py --profile-row blobs
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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_distance import fmt, make_map, once  # noqa: E402

ROWS = ("blobs", "noise", "ones", "stack", "cldice")
BAR_ROWS = ("blobs", "stack", "cldice")
ROW_LIMIT_S = {"blobs": 1500, "noise": 400, "ones": 900, "stack": 1200, "cldice": 6000}
KEPT_MARKER = "==== kept by tools/bench_skeleton.py"
CLASSES = [0, 1, 2, 3]


def make_row(row, edge, dev):
    if row == "ones":
        return torch.ones((edge, edge), dtype=torch.uint8, device=dev)
    return make_map("blobs" if row == "cldice" else row, edge, 0, dev)[0]


def chain_thin(mask):
    """guo_hall on a bool tensor [N, H, W] with torch ops: ``(skeleton, iterations)``"""
    s = mask.clone()
    H, W = s.shape[-2:]
    done = 0
    while True:
        any_deleted = torch.zeros((), dtype=torch.bool, device=s.device)
        for k in (0, 1):
            p = F.pad(s, (1, 1, 1, 1))
            P2, P3, P4, P5, P6, P7, P8, P9 = (p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in
                                              ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1)))
            u8 = torch.uint8
            c = (~P2 & (P3 | P4)).to(u8) + (~P4 & (P5 | P6)).to(u8) + (~P6 & (P7 | P8)).to(u8) + (~P8 & (P9 | P2)).to(u8)
            n1 = (P9 | P2).to(u8) + (P3 | P4).to(u8) + (P5 | P6).to(u8) + (P7 | P8).to(u8)
            n2 = (P2 | P3).to(u8) + (P4 | P5).to(u8) + (P6 | P7).to(u8) + (P8 | P9).to(u8)
            n = torch.minimum(n1, n2)
            m = (P6 | P7 | ~P9) & P8 if k == 0 else (P2 | P3 | ~P5) & P4
            d = s & (c == 1) & (n >= 2) & (n <= 3) & ~m
            any_deleted |= d.any()
            s = s & ~d
        if not bool(any_deleted):                       # the read-back of the iteration
            return s, done
        done += 1


def run_row(row, args):
    """one row in this process; prints its lines and a last line of JSON for the parent"""
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import centerline_dice, skeletonize

    dev = torch.device("cuda:0")
    labels = make_row(row, args.edge, dev)
    host_repeats = args.cldice_host_repeats if row == "cldice" else args.host_repeats
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    if row == "cldice":
        truth = torch.roll(labels, (3, 5), (-2, -1))

        def side_a():
            return centerline_dice(labels, truth, labels=CLASSES)["counts"]

        def side_h():
            return centerline_dice(labels.cpu(), truth.cpu(), labels=CLASSES)["counts"].to(dev)

        def side_c():
            masks = torch.stack([t == v for t in (labels, truth) for v in CLASSES])
            skel = chain_thin(masks)[0]
            K = len(CLASSES)
            return torch.stack([(skel[:K] & masks[K:]).sum((-1, -2)), skel[:K].sum((-1, -2)), (skel[K:] & masks[:K]).sum((-1, -2)), skel[K:].sum((-1, -2))], -1)

        got = side_a()
        iterations = None
        what = f"centerline_dice, {len(CLASSES)} classes"
    else:
        def side_a():
            return skeletonize(labels)

        def side_h():
            return skeletonize(labels.cpu()).to(dev)

        def side_c():
            return chain_thin((labels != 0).reshape((-1,) + labels.shape[-2:]))[0].reshape(labels.shape)

        got, iterations = skeletonize(labels, return_iterations=True)
        what = "skeletonize"
    torch.cuda.synchronize()
    sides = ["a", "c"] + ([] if row == "ones" else ["h"])
    times = {k: [] for k in sides}
    same = {}
    for k, fn in (("h", side_h), ("c", side_c)):
        if k in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = fn()
            torch.cuda.synchronize()
            first = time.perf_counter() - t0
            same[k] = bool(torch.equal(ref, got))
            if k == "h" and host_repeats == 0:
                times["h"].append(first)
            del ref
    say(f"{row}: {list(labels.shape)} {labels.dtype}: {int((labels != 0).sum())} of {labels.numel()} positions set"
        + (f", {int(got.sum())} in the skeleton after {iterations} iterations" if iterations is not None else f", counts of class 1: {got[1].tolist()}"))
    say("  " + "; ".join(f"(a) {'equals' if ok else '**DIFFERS FROM**'} ({k}) bit for bit" for k, ok in same.items()))
    fns = {"a": side_a, "h": side_h, "c": side_c}
    once(side_a)
    few = row not in BAR_ROWS                               # without a bar: the slow sides get three repeats
    for r in range(args.repeats):
        order = sides if r % 2 == 0 else sides[::-1]
        for k in order:
            if k == "h" and r >= host_repeats:
                continue
            if k == "c" and few and r >= 3:
                continue
            times[k].append(once(fns[k]))
    tm = {k: np.array(v) for k, v in times.items()}
    names = {"a": what, "h": "D2H + the library's CPU form + H2D (STAND-IN)", "c": "the formulae as a chain of torch ops on the device"}
    for k in sides:
        say(f"  ({k}) {names[k]:52s} {fmt(tm[k])}  [{len(tm[k])} samples]")
    if row == "ones":
        say("  (h) not run: the CPU form takes about as long per iteration as on the blob row, and this row has edge / 2 iterations")
    met, open_sides = None, []
    if row in BAR_ROWS:
        met = all(same.values())
        for k in ("h", "c"):
            gap = float(np.median(tm[k]) - np.median(tm["a"]))
            if len(tm[k]) < 3:                          # no spread to speak of: reported, the bar is not established on this side
                open_sides.append(k)
                say(f"  **({k}) - (a) = {gap * 1e3:.3f} ms from {len(tm[k])} sample of ({k}): no spread, the ({k}) half of the bar is NOT established on this row "
                    f"(({k}) / (a) = {np.median(tm[k]) / np.median(tm['a']):.1f})**")
                continue
            spread = float(max(np.ptp(tm["a"]), np.ptp(tm[k])))
            ok = gap > spread
            met = met and ok
            text = (f"({k}) - (a) = {gap * 1e3:.3f} ms, larger spread {spread * 1e3:.3f} ms: (a) {'beats' if ok else 'does NOT beat'} ({k}) by more than the spread "
                    f"(({k}) / (a) = {np.median(tm[k]) / np.median(tm['a']):.1f})")
            say("  " + (text if ok else f"**{text}**"))
    print("RESULT " + json.dumps({"row": row, "median_a": float(np.median(tm["a"])), "iterations": iterations, "bar": met, "open": open_sides, "lines": lines}), flush=True)


def profile_row(row, args):
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import skeletonize

    labels = make_row(row, args.edge, torch.device("cuda:0"))
    for _ in range(4):                       # (one warm-up and three calls; the per-kernel SHARES are what is read from the trace)
        skeletonize(labels)
    torch.cuda.synchronize()


def write_out(path, lines):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        kept = kept_sections(path)
        with open(path, "w") as f:
            f.write("\n".join(lines + ([""] + kept if kept else [])) + "\n")


def steps_row(args):
    """one line: skeletonize on the blob row with the library that is loaded (PTB_HIP_LIB), 7 repeats after a warm-up"""
    import __graft_entry__ as g

    if not os.environ.get("PTB_HIP_LIB"):
        g.build()
    from pytorch_toolbelt_amd import _native as N
    from pytorch_toolbelt_amd.utils import skeletonize

    labels = make_row("blobs", args.edge, torch.device("cuda:0"))
    got, n = skeletonize(labels, return_iterations=True)
    once(lambda: skeletonize(labels))
    t = np.array([once(lambda: skeletonize(labels)) for _ in range(args.repeats)])
    print(f"STEPS = {N.load().ptb_thin_steps():2d}: blobs {args.edge} x {args.edge}, {n} iterations, {int(got.sum())} skeleton positions: {fmt(t)}", flush=True)


def kept_sections(path):
    """the lines of an existing file from KEPT_MARKER on"""
    try:
        old = open(path).read().splitlines()
    except OSError:
        return []
    at = [i for i, ln in enumerate(old) if ln.startswith(KEPT_MARKER)]
    return old[at[0]:] if at else []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=None)
    ap.add_argument("--edge", type=int, default=5000)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", help="(internal) run one row in this process")
    ap.add_argument("--cldice-host-repeats", type=int, default=None)
    ap.add_argument("--profile-row", choices=ROWS)
    ap.add_argument("--steps-row", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skeleton_bench.txt"))
    args = ap.parse_args()
    if args.host_repeats is None:
        args.host_repeats = args.repeats
    if args.cldice_host_repeats is None:
        args.cldice_host_repeats = args.host_repeats
    if args.repeats < 7 or not 3 <= args.host_repeats <= args.repeats or not 0 <= args.cldice_host_repeats <= args.repeats:
        sys.exit("bench_skeleton: at least 7 repeats, between 3 and --repeats host repeats, and between 0 and --repeats for the cldice row")
    if not torch.cuda.is_available():
        sys.exit("bench_skeleton: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    if args.profile_row:
        return profile_row(args.profile_row, args)
    if args.steps_row:
        return steps_row(args)
    if args.row:
        return run_row(args.row, args)
    lines = [f"skeletonize and centerline_dice (guo_hall) on {torch.cuda.get_device_name(0)}, edge {args.edge}; {args.repeats} alternating repeats (order reversed every round; "
             f"the host side (h) in {args.host_repeats} of them, on the cldice row in {args.cldice_host_repeats}"
             + (": there its one compared call is its only sample" if args.cldice_host_repeats == 0 else "") + ") after 1 warm-up run of every side; host clock around device-synchronised calls; every row in a process of its own under its own time limit"]
    print(lines[0], flush=True)
    results, failed = {}, None
    rows = args.rows.split(",")
    for row in rows:
        cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--repeats", str(args.repeats), "--host-repeats", str(args.host_repeats), "--edge", str(args.edge),
               "--cldice-host-repeats", str(args.cldice_host_repeats)]
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
        write_out(args.out, lines + [f"(rows still to run: {rows[rows.index(row) + 1:]})"])
    if failed:
        lines.append("**" + failed + "**")
    have = [r for r in BAR_ROWS if r in results]
    if failed or len(have) < len(BAR_ROWS):
        lines.append(f"THE BAR: **not established: of the rows {BAR_ROWS} only {tuple(have)} ran here**" + (f"; on those: {[(r, results[r]['bar']) for r in have]}" if have else ""))
    else:
        lines.append("THE BAR ((a) beats (h) and (c) on blobs, stack and cldice by more than the spread): "
                     + ("met" if all(results[r]["bar"] for r in BAR_ROWS) else "**NOT met**") + f" {[(r, results[r]['bar']) for r in BAR_ROWS]}"
                     + "".join(f"; **on {r} only for the sides measured: the ({'), ('.join(results[r]['open'])}) half has fewer than 3 samples and is NOT established**"
                               for r in BAR_ROWS if results[r]["open"]))
    print(lines[-1], flush=True)
    write_out(args.out, lines)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
