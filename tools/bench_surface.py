#!/usr/bin/env python3
"""Benchmark of the surface metrics on one MI355X (utils/surface.py, csrc/ptb_surface.hip).

Inputs, seeded and generated here, uint8, K = 4 classes (labels 0..3, every one scored as an object).  5000 x 5000: a 4-class blob map as
merge_crop(argmax=True, dtype=torch.uint8) leaves it is the truth; pred is the truth rolled by (3, 5) pixels with every 17th connected
component dropped (set to class 0).  The same size with noise: the truth holds a random class 1..3 on a random half of the positions
and 0 elsewhere, pred re-draws 5 % of the positions.  A 256^3 and a 512^3 4-class blob volume pair (pred rolled by (1, 3, 5)).

Timed, each call from its start to a device synchronise behind its last piece of work, after a warm-up of every side, in rounds that
alternate between the sides (the order inside a round turns over every round):
  (a) surface_metrics(pred, truth, (0, 1, 2, 3), tolerance=(1, 2))  -- nothing read back
  (h) the host route: D2H of both maps, then per class the scipy recipe (binary_erosion, distance_transform_edt, np.percentile,
      np.mean, counts); nothing copied back.  Left out for 512^3 (8 scipy transforms of 512^3 are about two minutes per repeat).
  (c) the composed device route, torch ops and this library's distance_transform only: per class two boolean masks, two erosions out
      of pooling ops, two distance_transform calls, two boolean gathers (a host synchronisation each), max / mean / counts and the
      percentile by torch.quantile, or by torch.sort where a set has more than 16 M samples, which quantile refuses.  2-D rows only.
Context, in the same process: the 2 K distance_transform calls of the border maps one by one (t) against ONE call on their stack (s)
-- the batching argument -- and the copy rate.  Nothing is claimed as a share of peak: the work is latency- and atomic-bound.
THE BAR: (a) beats (h) by more than the larger spread on the blob maps, the noise maps and the 256^3 volume.  (c) is reported only; a row
on which (a) does not beat it by more than the spread is printed in bold.

Every row runs in a child process of its own under its own time limit; after a row that fails or runs out of time nothing more is started.

    python tools/bench_surface.py [--repeats 7] [--edge 5000] [--out profiles/surface_bench.txt]
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

ROWS = ("blobs", "noise", "volume256", "volume512")
BARRED = ("blobs", "noise", "volume256")
ROW_LIMIT_S = {"blobs": 420, "noise": 540, "volume256": 540, "volume512": 240}
LABELS = (0, 1, 2, 3)
TOLERANCES = (1.0, 2.0)
PERCENTILE = 95.0
BIG_WORKSPACE = 24 << 30         # 512^3: one class is 4.6 GB of workspace, above the default cap of 4 GiB; all four are 18.3 GB


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def alternate(sides, repeats):
    times = {k: [] for k in sides}
    order = list(sides)
    for r in range(repeats):
        for k in (order if r % 2 == 0 else order[::-1]):
            times[k].append(once(sides[k]))
    return {k: np.array(v) for k, v in times.items()}


def copy_rate(dev):
    """bytes per second (read + written) of a 256 MB device-to-device copy, the median of 5"""
    src = torch.empty(64 << 20, dtype=torch.int32, device=dev)
    dst = torch.empty_like(src)
    once(lambda: dst.copy_(src))
    t = np.median([once(lambda: dst.copy_(src)) for _ in range(5)])
    return 2 * src.numel() * 4 / t


def make_pair(row, edge, dev):
    """(pred, truth, dims)"""
    from bench_metrics import blob_labels
    from pytorch_toolbelt_amd.utils import connected_components

    if row == "blobs":
        truth = blob_labels((edge, edge), 4, 0, dev)
        pred = torch.roll(truth, shifts=(3, 5), dims=(-2, -1)).clone()
        cc, _ = connected_components(pred, connectivity=4, background=None)
        pred[cc % 17 == 3] = 0
        return pred, truth, 2
    if row == "noise":
        g = torch.Generator().manual_seed(1)
        truth = (torch.randint(1, 4, (edge, edge), generator=g, dtype=torch.uint8) * torch.randint(0, 2, (edge, edge), generator=g, dtype=torch.uint8)).to(dev)
        redraw = (torch.rand((edge, edge), generator=g) < 0.05).to(dev)
        other = torch.randint(0, 4, (edge, edge), generator=g, dtype=torch.uint8).to(dev)
        return torch.where(redraw, other, truth), truth, 2
    cube = 256 if row == "volume256" else 512
    truth = blob_labels((cube,) * 3, 4, 2, dev)
    return torch.roll(truth, shifts=(1, 3, 5), dims=(-3, -2, -1)).clone(), truth, 3


# ---------------------------------------------------------------------------------------------------------------- (h)
def host_route(pred, truth, dims):
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure

    p, t = pred.cpu().numpy(), truth.cpu().numpy()
    st = generate_binary_structure(dims, 1)
    out = []
    for c in LABELS:
        a, b = p == c, t == c
        ba, bb = a ^ binary_erosion(a, st), b ^ binary_erosion(b, st)
        d0 = distance_transform_edt(~bb)[ba] if bb.any() else np.full(int(ba.sum()), np.inf)
        d1 = distance_transform_edt(~ba)[bb] if ba.any() else np.full(int(bb.sum()), np.inf)
        pooled = np.concatenate([d0, d1])
        out.append(dict(hausdorff=max(d0.max(), d1.max()), hausdorff_percentile=np.percentile(pooled, PERCENTILE), assd=(d0.mean() + d1.mean()) / 2,
                        surface_dice=[float((pooled <= tol).sum()) / len(pooled) for tol in TOLERANCES]))
    return out


# ---------------------------------------------------------------------------------------------------------------- (c)
def border_2d(mask):
    """mask ^ its 4-connected erosion (outside the map counts as background), from pooling ops"""
    x = F.pad(mask[None, None].to(torch.float16), (1, 1, 1, 1))
    inv = 1 - x
    grown = torch.maximum(F.max_pool2d(inv, (3, 1), 1)[..., 1:-1], F.max_pool2d(inv, (1, 3), 1)[..., 1:-1, :])
    return mask & (grown[0, 0] > 0)


def quantile(d, q):
    if d.numel() <= 16_000_000:
        return torch.quantile(d, q)
    s = torch.sort(d).values
    pos = (d.numel() - 1) * q
    lo = int(pos)
    return s[lo] + (s[min(lo + 1, d.numel() - 1)] - s[lo]) * (pos - lo)


def composed_route(pred, truth):
    from pytorch_toolbelt_amd.utils import distance_transform

    out = []
    for c in LABELS:
        ba, bb = border_2d(pred == c), border_2d(truth == c)
        da, db = distance_transform(ba.to(torch.uint8), foreground=0), distance_transform(bb.to(torch.uint8), foreground=0)
        d0, d1 = db[ba], da[bb]
        pooled = torch.cat([d0, d1])
        out.append(dict(hausdorff=torch.maximum(d0.max(), d1.max()), hausdorff_percentile=quantile(pooled, PERCENTILE / 100), assd=(d0.mean() + d1.mean()) / 2,
                        surface_dice=[(pooled <= tol).sum() / pooled.numel() for tol in TOLERANCES]))
    return out


def fmt(t):
    return f"{np.median(t) * 1e3:10.3f} ms (spread {(t.max() - t.min()) * 1e3:8.3f} ms)"


def differs(res, other):
    """largest relative difference of the symmetric results of (a) against another side's list of per-class dicts"""
    worst = 0.0
    for k, o in enumerate(other):
        for key in ("hausdorff", "hausdorff_percentile", "assd"):
            a, b = float(res[key][k]), float(o[key])
            worst = max(worst, abs(a - b) / max(abs(b), 1e-30))
        for i in range(len(TOLERANCES)):
            a, b = float(res["surface_dice"][k, i]), float(o["surface_dice"][i])
            worst = max(worst, abs(a - b) / max(abs(b), 1e-30))
    return worst


def run_row(row, args):
    """one row in this process; prints its lines and a last line of JSON for the parent"""
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import distance_transform, surface_metrics
    from pytorch_toolbelt_amd.utils.surface import _workspace_plan as workspace_plan

    dev = torch.device("cuda:0")
    pred, truth, dims = make_pair(row, args.edge, dev)
    rate = copy_rate(dev)
    cap = BIG_WORKSPACE if row == "volume512" else None
    plan = workspace_plan(pred.shape, len(LABELS), dims, cap)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def side_a():
        return surface_metrics(pred, truth, LABELS, dims=dims, percentile=PERCENTILE, tolerance=TOLERANCES, max_workspace_bytes=cap)

    res = side_a()
    torch.cuda.synchronize()
    say(f"{row}: {list(pred.shape)} uint8 pair, dims={dims}, K={len(LABELS)}: {res['surface_count'].sum(0).tolist()} surface positions (pred, truth), "
        f"hausdorff {[round(float(v), 2) for v in res['hausdorff']]}, hd95 {[round(float(v), 2) for v in res['hausdorff_percentile']]}, "
        f"assd {[round(float(v), 3) for v in res['assd']]}; {plan['chunk']} classes per chunk, workspace {plan['bytes'] / 1e9:.2f} GB"
        f"{'' if cap is None else ' (max_workspace_bytes=24 GiB: one class alone passes the default cap)'}; copy rate here {rate / 1e12:.2f} TB/s")
    sides = {"a": side_a}
    if row != "volume512":
        try:
            import scipy.ndimage  # noqa: F401

            sides["h"] = lambda: host_route(pred, truth, dims)
        except ImportError:
            say("  (h) left out: scipy is not installed on this machine")
    if dims == 2:
        sides["c"] = lambda: composed_route(pred, truth)
    for k in ("h", "c"):
        if k in sides:
            t0 = time.perf_counter()
            other = sides[k]()                                # (the side's warm-up is also the result that is compared)
            torch.cuda.synchronize()
            worst = differs(res, other)
            say(f"  ({k}) first call {time.perf_counter() - t0:.1f} s; (a) against ({k}): largest relative difference of hausdorff, hd95, assd, surface Dice "
                f"{worst:.2e}: {'equal within 1e-5' if worst <= 1e-5 else '**DIFFERENT**'}")
            del other
    tm = alternate(sides, args.repeats)
    names = {"a": "surface_metrics", "h": "D2H + scipy recipe per class", "c": "torch ops + distance_transform per class"}
    for k, t in tm.items():
        say(f"  ({k}) {names[k]:42s} {fmt(t)}")
    result = {"row": row, "median_a": float(np.median(tm["a"])), "bar": None}
    for k in ("h", "c"):
        if k not in tm:
            continue
        gap = float(np.median(tm[k]) - np.median(tm["a"]))
        spread = float(max(np.ptp(tm["a"]), np.ptp(tm[k])))
        met = gap > spread
        text = (f"({k}) - (a) = {gap * 1e3:.3f} ms, larger spread {spread * 1e3:.3f} ms: (a) {'beats' if met else 'does NOT beat'} ({k}) by more than the spread "
                f"(({k}) / (a) = {np.median(tm[k]) / np.median(tm['a']):.1f})")
        barred = k == "h" and row in BARRED
        say("  " + (text if met else f"**{text}**") + ("" if barred else "   [reported, not barred]"))
        if barred:
            result["bar"] = met
    # context: the transforms of the 2 K border maps one by one against one call on their stack
    if dims == 2:
        borders = torch.stack([border_2d(m == c) for c in LABELS for m in (pred, truth)]).to(torch.uint8)
    else:
        borders = None
    if borders is not None:
        ctx = alternate({"t": lambda: [distance_transform(b, foreground=0, squared=True) for b in borders],
                         "s": lambda: distance_transform(borders, foreground=0, squared=True)}, args.repeats)
        say(f"  (t) {2 * len(LABELS)} distance_transform calls, map by map      {fmt(ctx['t'])}")
        say(f"  (s) one distance_transform of their stack       {fmt(ctx['s'])}   (t) / (s) = {np.median(ctx['t']) / np.median(ctx['s']):.2f}; "
            f"(a) / (t) = {np.median(tm['a']) / np.median(ctx['t']):.2f}")
    result["lines"] = lines
    print("RESULT " + json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--edge", type=int, default=5000)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", help="(internal) run one row in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_bench.txt"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("bench_surface: at least 7 repeats")
    if not torch.cuda.is_available():
        sys.exit("bench_surface: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    if args.row:
        return run_row(args.row, args)
    lines = [f"surface metrics on {torch.cuda.get_device_name(0)}; {args.repeats} alternating repeats (order reversed every round) after 1 warm-up run "
             "of every side; host clock around device-synchronised calls; every row in a process of its own under its own time limit"]
    print(lines[0], flush=True)
    results, failed = {}, None
    for row in args.rows.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--repeats", str(args.repeats), "--edge", str(args.edge)]
        child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)     # (one pipe, read as it fills: nothing can block the child)
        timed_out = []
        timer = threading.Timer(ROW_LIMIT_S[row], lambda: (timed_out.append(True), child.kill()))
        timer.start()
        stdout = []
        for ln in child.stdout:                       # (echoed as it comes: a long row is not a silent one)
            stdout.append(ln.rstrip("\n"))
            if not ln.startswith("RESULT "):
                print(ln, end="", flush=True)
        child.wait()
        timer.cancel()
        if timed_out:
            failed = f"{row}: no result within its time limit of {ROW_LIMIT_S[row]} s; nothing more was started"
            break
        res = [ln for ln in stdout if ln.startswith("RESULT ")]
        if child.returncode != 0 or not res:
            failed = f"{row}: exit status {child.returncode}; nothing more was started\n" + "\n".join(stdout)[-2000:]
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
        lines.append("THE BAR ((a) beats the host route on the blob maps, the noise maps and the 256^3 volume by more than the spread): "
                     + ("met" if all(results[r]["bar"] for r in BARRED) else "**NOT met**") + f" {[(r, results[r]['bar']) for r in BARRED]}")
    print("\n".join(lines[-3:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
