#!/usr/bin/env python3
"""Benchmark of the hard-example-mining losses on one MI355X (losses/hard_mining.py, csrc/ptb_hard_mining.hip).

Inputs, seeded and generated here: logits N(0, 2), uniform random labels (multiclass) or 0 / 1 targets (binary) --
  cfg4_topk    [32, 16, 512, 512] multiclass (the bench.py cfg4 shape), top-k 10 %
  cfg4_ohem    the same, OHEM thresh 0.7 / min_kept 100 000
  b8c4_topk    [8, 4, 512, 512] multiclass, top-k 10 %
  volume_topk  [2, 3, 128, 128, 128] multiclass, top-k 10 %
  binary_topk  [8, 1, 512, 512] binary, top-k 10 %

Timed, each call -- forward, backward, to a device synchronise behind the gradient -- after three warm-up runs of every side (measured here:
the second call of either side, the device form and the torch chain alike, is still 0.3 - 0.6 ms above the later ones, so one warm-up
run puts that into the first timed repeat), in rounds that alternate between the sides (the order inside a round turns over every round):
  (a) TopKCrossEntropyLoss / OhemCrossEntropyLoss
  (t) the torch chain on the device: F.cross_entropy (F.binary_cross_entropy_with_logits) reduction="none" -> flatten -> topk -> mean;
      OHEM rows: -> sort, keep what lies above t0 or among the min_kept largest, masked mean (no read-back either)
Reported per row: median and spread (max - min) of the repeats, the relative difference of the two loss values and of the gradients.
THE BAR, per multiclass row: (a) is ahead of (t) by more than the larger spread of the two sides.  The binary row is reported.
For information, without a bar: the copy rate of the same process (a 256 MB device-to-device copy) and the time the bytes of the loss
pass -- logits and target read once, the 4-byte map written -- would take at that rate; the kernel's own time is in the trace below.

Every row runs in a child process of its own under its own time limit; after a row that fails or runs out of time nothing more is
started.  --profile-row NAME runs the row's (a) four times, for a per-kernel trace from outside.

    python tools/bench_hard_mining.py [--repeats 7] [--out profiles/hard_mining_bench.txt]
"""
import argparse
import json
import math
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

from bench_distance import alternate, copy_rate, fmt  # noqa: E402

#            mode          B   C  spatial          rule
ROWS = {"cfg4_topk": ("multiclass", 32, 16, (512, 512), "topk"), "cfg4_ohem": ("multiclass", 32, 16, (512, 512), "ohem"),
        "b8c4_topk": ("multiclass", 8, 4, (512, 512), "topk"), "volume_topk": ("multiclass", 2, 3, (128, 128, 128), "topk"),
        "binary_topk": ("binary", 8, 1, (512, 512), "topk")}
BARRED = tuple(r for r, v in ROWS.items() if v[0] == "multiclass")
ROW_LIMIT_S = 240
WARMUP = 3          # runs of every side before the timed ones: the SECOND call of either side still takes 0.3 - 0.6 ms longer than the later ones
K_PERCENT, THRESH, MIN_KEPT = 10.0, 0.7, 100_000


def make_inputs(row, dev):
    mode, B, C, spatial, _ = ROWS[row]
    g = torch.Generator().manual_seed(5)
    x = (2.0 * torch.randn((B, C) + spatial, generator=g)).to(dev)
    if mode == "multiclass":
        t = torch.randint(0, C, (B,) + spatial, generator=g).to(dev)
    else:
        t = torch.randint(0, 2, (B, C) + spatial, generator=g).float().to(dev)
    return x, t


def criterion(row):
    from pytorch_toolbelt_amd import losses

    mode, _, _, _, rule = ROWS[row]
    return losses.TopKCrossEntropyLoss(mode, k=K_PERCENT) if rule == "topk" else losses.OhemCrossEntropyLoss(mode, thresh=THRESH, min_kept=MIN_KEPT)


def torch_chain(row, x, t):
    mode, _, _, _, rule = ROWS[row]
    l = (F.cross_entropy(x, t, reduction="none") if mode == "multiclass" else F.binary_cross_entropy_with_logits(x, t, reduction="none")).flatten()
    n = l.numel()
    if rule == "topk":
        return l.topk(max(1, int(n * K_PERCENT / 100)))[0].mean()
    t0 = float(np.float32(-math.log(THRESH)))
    floor = l.detach().sort(descending=True)[0][min(MIN_KEPT, n) - 1]
    keep = (l.detach() > t0) | (l.detach() >= floor)
    return (l * keep).sum() / keep.sum()


def run_row(row, args):
    """one row in this process; prints its lines and a last line of JSON for the parent"""
    import __graft_entry__ as g

    g.build()
    dev = torch.device("cuda:0")
    mode, B, C, spatial, rule = ROWS[row]
    x, t = make_inputs(row, dev)
    x.requires_grad_(True)
    crit = criterion(row)
    lines, values = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def finish(name, loss):
        x.grad = None
        loss.backward()
        values[name] = loss.detach()
        return x.grad

    sides = {"a": lambda: finish("a", crit(x, t)), "t": lambda: finish("t", torch_chain(row, x, t))}
    what = f"top-k {K_PERCENT:g} %" if rule == "topk" else f"OHEM thresh {THRESH} / min_kept {MIN_KEPT}"
    say(f"{row}: logits {list(x.shape)} fp32, target {list(t.shape)} {str(t.dtype).split('.')[1]}, {mode}, {what}")
    grads = {k: f().clone() for k, f in sides.items()}            # (the warm-up of every side is the call whose result is compared)
    torch.cuda.synchronize()
    ref = float(values["a"])
    gd = float((grads["t"] - grads["a"]).abs().max() / grads["a"].abs().max())
    say(f"  (t) against (a): loss {float(values['t']):.7g} against {ref:.7g} (relative {abs(float(values['t']) - ref) / max(abs(ref), 1e-30):.1e}), "
        f"largest gradient difference / largest gradient {gd:.1e}")
    del grads
    for _ in range(WARMUP - 1):                                   # (further warm-up rounds, alternating like the timed ones)
        for f in sides.values():
            f()
    torch.cuda.synchronize()
    tm = alternate(sides, args.repeats)
    names = {"a": f"{type(crit).__name__} forward + backward", "t": "cross-entropy none -> " + ("topk -> mean" if rule == "topk" else "sort -> masked mean")}
    for k, v in tm.items():
        say(f"  ({k}) {names[k]:52s} {fmt(v)}")
        say(f"      the repeats in order, ms: {' '.join(f'{1e3 * r:.3f}' for r in v)}")
    gap = float(np.median(tm["t"]) - np.median(tm["a"]))
    spread = float(max(np.ptp(tm["a"]), np.ptp(tm["t"])))
    ok = gap > spread
    text = (f"(t) - (a) = {gap * 1e3:.3f} ms, larger spread {spread * 1e3:.3f} ms: (a) is {'ahead' if ok else 'NOT ahead'} of (t) by more than the spread "
            f"((t) / (a) = {np.median(tm['t']) / np.median(tm['a']):.1f})" + ("" if row in BARRED else "   [reported, not barred]"))
    say("  " + (text if ok else f"**{text}**"))
    rate = copy_rate(dev)
    elements = t.numel()
    moved = x.numel() * 4 + t.numel() * t.element_size() + elements * 4
    say(f"  copy rate of this process {rate / 1e12:.2f} TB/s; the loss pass moves {moved / 2 ** 20:.0f} MiB (logits, target, the 4-byte map): "
        f"{moved / rate * 1e6:.0f} us at that rate   [information, no bar]")
    print("RESULT " + json.dumps({"row": row, "median_a": float(np.median(tm["a"])), "bar": bool(ok), "lines": lines}), flush=True)


def profile_row(row, args):
    import __graft_entry__ as g

    g.build()
    dev = torch.device("cuda:0")
    x, t = make_inputs(row, dev)
    x.requires_grad_(True)
    crit = criterion(row)
    for _ in range(4):                       # (one warm-up and three calls; the per-kernel SHARES are what is read from the trace)
        x.grad = None
        crit(x, t).backward()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", help="(internal) run one row in this process")
    ap.add_argument("--profile-row", choices=tuple(ROWS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hard_mining_bench.txt"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("bench_hard_mining: at least 7 repeats")
    if not torch.cuda.is_available():
        sys.exit("bench_hard_mining: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    if args.profile_row:
        return profile_row(args.profile_row, args)
    if args.row:
        return run_row(args.row, args)
    lines = [f"hard-example mining on {torch.cuda.get_device_name(0)}; forward + backward, {args.repeats} alternating repeats (order reversed every round) after {WARMUP} "
             "warm-up runs of every side; host clock around device-synchronised calls; every row in a process of its own under its own time limit"]
    print(lines[0], flush=True)
    results, failed = {}, None
    rows = args.rows.split(",")
    for row in rows:
        cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--repeats", str(args.repeats)]
        child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        timed_out = []
        timer = threading.Timer(ROW_LIMIT_S, lambda: (timed_out.append(True), child.kill()))
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
            failed = f"{row}: no result within its time limit of {ROW_LIMIT_S} s; nothing more was started"
            break
        res = [ln for ln in stdout if ln.startswith("RESULT ")]
        if child.returncode != 0 or not res:
            failed = f"{row}: exit status {child.returncode}; nothing more was started\n" + stderr[-2000:]
            break
        results[row] = json.loads(res[-1][7:])
        lines += results[row]["lines"]
    if failed:
        lines.append("**" + failed + "**")
    have = [r for r in rows if r in results]
    if failed or any(r not in results for r in BARRED):
        lines.append(f"THE BAR: **not established: of the rows {tuple(ROWS)} only {tuple(have)} ran here**" + (f"; on those: {[(r, results[r]['bar']) for r in have]}" if have else ""))
    else:
        lines.append("THE BAR (on every multiclass row the device form is ahead of the torch chain by more than the larger spread): "
                     + ("met" if all(results[r]["bar"] for r in BARRED) else "**NOT met**") + f" {[(r, results[r]['bar']) for r in BARRED]}")
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
