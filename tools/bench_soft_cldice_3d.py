#!/usr/bin/env python3
"""Benchmark of SoftClDiceLoss(dims=3), forward + backward, on one MI355X (losses/cldice.py, csrc/ptb_softskel3d.hip).

Rows (seeded random logits and targets, generated outside the timed region):
  binary-k3       [2, 1, 128, 128, 128] binary,                        iterations = 3
  multiclass-k3   [2, 3, 128, 128, 128] multiclass, classes = [1, 2],  iterations = 3
  multiclass-k8   [2, 3, 128, 128, 128] multiclass, classes = [1, 2],  iterations = 8      (reported without a bar)

Timed, each call from its start to a device synchronise behind its last piece of work, after two warm-up calls of every side, in rounds that
alternate between the sides (the order inside a round turns over every round):
  (a) the loss of this library and its backward
  (c) the same definition as a chain of torch ops on the device (max_pool3d / relu) with autograd -- what a user had before
The peak device memory of one call of each side (above what the inputs hold) is reported next to the times.
THE BAR: on the two k = 3 rows (a) beats (c) by more than the larger spread of the two sides.  A row that misses is printed in bold.
Every row runs in a child process of its own under its own time limit; after a row that fails nothing more is started.

    python tools/bench_soft_cldice_3d.py [--repeats 7] [--out profiles/soft_cldice_3d_bench.txt]

The kernel-time split of a row: --profile-row NAME runs the row's (a) three times after one warm-up, for
    rocprofv3 --kernel-trace --stats -- python tools/bench_soft_cldice_3d.py --profile-row binary-k3
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_distance import fmt, once  # noqa: E402

ROWS = {"binary-k3": ("binary", 1, 3), "multiclass-k3": ("multiclass", 3, 3), "multiclass-k8": ("multiclass", 3, 8)}
BAR_ROWS = ("binary-k3", "multiclass-k3")
ROW_LIMIT_S = 300
B, EDGE = 2, 128
CLASSES = [1, 2]                                  # of the multiclass rows


def make_row(row, dev):
    mode, C, k = ROWS[row]
    gen = torch.Generator().manual_seed(0)
    x = torch.randn((B, C, EDGE, EDGE, EDGE), generator=gen).to(dev)
    y = (torch.rand((B, 1, EDGE, EDGE, EDGE), generator=gen) > 0.5).float() if mode == "binary" else torch.randint(0, C, (B, EDGE, EDGE, EDGE), generator=gen)
    return mode, k, x, y.to(dev)


def chain_loss(x, y, mode, k, smooth=1.0):
    """the dims=3 definition of losses/cldice.py as torch ops"""
    def skeleton(v):
        skel = None
        for _ in range(k + 1):
            nxt = -torch.maximum(torch.maximum(F.max_pool3d(-v, (3, 1, 1), 1, (1, 0, 0)), F.max_pool3d(-v, (1, 3, 1), 1, (0, 1, 0))),
                                 F.max_pool3d(-v, (1, 1, 3), 1, (0, 0, 1)))
            delta = F.relu(v - F.max_pool3d(nxt, 3, 1, 1))
            skel = delta if skel is None else skel + F.relu(delta - skel * delta)
            v = nxt
        return skel

    p = torch.sigmoid(x) if mode == "binary" else torch.softmax(x, 1)[:, CLASSES]
    g = y if mode == "binary" else F.one_hot(y, x.shape[1]).permute(0, 4, 1, 2, 3)[:, CLASSES].float()
    sp, st = skeleton(p), skeleton(g)
    tprec = ((sp * g).sum((0, 2, 3, 4)) + smooth) / (sp.sum((0, 2, 3, 4)) + smooth)
    tsens = ((st * p).sum((0, 2, 3, 4)) + smooth) / (st.sum((0, 2, 3, 4)) + smooth)
    return (1.0 - 2.0 * tprec * tsens / (tprec + tsens)).mean()


def sides_of(row, dev):
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.losses import SoftClDiceLoss

    mode, k, x, y = make_row(row, dev)
    loss = SoftClDiceLoss(mode, classes=None if mode == "binary" else CLASSES, iterations=k, dims=3)

    def step(fn):
        leaf = x.detach().requires_grad_(True)
        out = fn(leaf)
        out.backward()
        return out.detach(), leaf.grad

    return {"a": lambda: step(lambda t: loss(t, y)), "c": lambda: step(lambda t: chain_loss(t, y, mode, k))}, x


def run_row(row, args):
    """one row in this process; prints its lines and a last line of JSON for the parent"""
    dev = torch.device("cuda:0")
    fns, x = sides_of(row, dev)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    first, peak = {}, {}
    for k, fn in fns.items():                               # the warm-up of every side; its result is compared, its peak memory kept
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        first[k] = fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - base
    top = float(first["c"][1].abs().max())
    say(f"{row}: {list(x.shape)} {ROWS[row][0]}, iterations = {ROWS[row][2]}: loss (a) {float(first['a'][0]):.7f}, (c) {float(first['c'][0]):.7f}; "
        f"max|grad (a) - grad (c)| / max|grad (c)| = {float((first['a'][1] - first['c'][1]).abs().max()) / top:.3e} (random logits: selections may differ where fp32 values tie)")
    del first
    for fn in fns.values():                                 # (a second warm-up: the first call of a side also fills the allocator's pool)
        once(fn)
    times = {k: [] for k in fns}
    for r in range(args.repeats):
        for k in (("a", "c") if r % 2 == 0 else ("c", "a")):
            times[k].append(once(fns[k]))
    tm = {k: np.array(v) for k, v in times.items()}
    names = {"a": "SoftClDiceLoss forward + backward", "c": "the chain of torch ops with autograd"}
    for k in fns:
        say(f"  ({k}) {names[k]:40s} {fmt(tm[k])}  peak memory {peak[k] / 2 ** 20:8.1f} MiB  [{len(tm[k])} samples]")
    gap, spread = float(np.median(tm["c"]) - np.median(tm["a"])), float(max(np.ptp(tm["a"]), np.ptp(tm["c"])))
    ok = gap > spread
    text = (f"(c) - (a) = {gap * 1e3:.3f} ms, larger spread {spread * 1e3:.3f} ms: (a) {'beats' if ok else 'does NOT beat'} (c) by more than the spread "
            f"((c) / (a) = {np.median(tm['c']) / np.median(tm['a']):.2f})" + ("" if row in BAR_ROWS else "  [no bar on this row]"))
    say("  " + (text if ok or row not in BAR_ROWS else f"**{text}**"))
    print("RESULT " + json.dumps({"row": row, "bar": ok, "lines": lines}), flush=True)


def profile_row(row):
    fns, _ = sides_of(row, torch.device("cuda:0"))
    for _ in range(4):                                      # (one warm-up and three calls: the last three dispatches of a kernel are the record)
        fns["a"]()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", help="(internal) run one row in this process")
    ap.add_argument("--profile-row", choices=tuple(ROWS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft_cldice_3d_bench.txt"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("bench_soft_cldice_3d: at least 7 repeats")
    if not torch.cuda.is_available():
        sys.exit("bench_soft_cldice_3d: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    if args.profile_row:
        return profile_row(args.profile_row)
    if args.row:
        return run_row(args.row, args)
    lines = [f"SoftClDiceLoss(dims=3) forward + backward on {torch.cuda.get_device_name(0)}; {args.repeats} alternating repeats (order reversed every round) after 2 warm-up runs "
             "of every side; host clock around device-synchronised calls; every row in a process of its own"]
    print(lines[0], flush=True)
    results, failed = {}, None
    for row in args.rows.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--repeats", str(args.repeats)]
        try:
            child = subprocess.run(cmd, capture_output=True, text=True, timeout=ROW_LIMIT_S)
        except subprocess.TimeoutExpired:
            failed = f"{row}: no result within its time limit of {ROW_LIMIT_S} s; nothing more was started"
            break
        res = [ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")]
        if child.returncode != 0 or not res:
            failed = f"{row}: exit status {child.returncode}; nothing more was started\n" + child.stderr[-2000:]
            break
        results[row] = json.loads(res[-1][7:])
        print("\n".join(results[row]["lines"]), flush=True)
        lines += results[row]["lines"]
    if failed:
        lines.append("**" + failed + "**")
    have = [r for r in BAR_ROWS if r in results]
    if failed or len(have) < len(BAR_ROWS):
        lines.append(f"THE BAR: **not established: of the rows {BAR_ROWS} only {tuple(have)} ran here**")
    else:
        lines.append("THE BAR ((a) beats (c) on the two k = 3 rows by more than the spread): " + ("met" if all(results[r]["bar"] for r in BAR_ROWS) else "**NOT met**")
                     + f" {[(r, results[r]['bar']) for r in BAR_ROWS]}")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
