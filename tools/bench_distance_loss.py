#!/usr/bin/env python3
"""Benchmark of the distance-map losses on one MI355X (losses/distance_losses.py, csrc/ptb_distance_loss.hip).

Inputs, seeded and generated here: multiclass logits N(0, 2) with blob label maps (tools/bench_metrics.blob_labels) --
  2d        [8, 4, 512, 512] logits, labels [8, 512, 512]
  3d        [2, 3, 128, 128, 128] logits, labels [2, 128, 128, 128]
Rows: forward + backward of BoundaryLoss and of HausdorffDTLoss (alpha = 2) on each, and BoundaryLoss on 2d with ``dist_maps=`` given
(``class_distance_maps(squared=True)``, made outside the timed region).

Timed, each call -- forward, backward, to a device synchronise behind the gradient -- after a warm-up of every side, in rounds that
alternate between the sides (the order inside a round turns over every round):
  (a) the fused path
  (h) what users do today: D2H of the labels (Hausdorff: and of the thresholded prediction), scipy.ndimage.distance_transform_edt per
      sample and class (object and complement, the ``if mask.any()`` rule), H2D, then torch softmax / multiply / mean with autograd
  (c) the composition on the device: ``distance_transform(signed=True)`` per class (Hausdorff: and per class of the thresholded
      prediction), inf -> 0, then the same torch ops with autograd
  (t) maps row only: the same torch ops on the given maps (reported, no bar)
Reported per row: median and spread (max - min) of the repeats and the relative difference of the three loss values.
THE BAR, per row: (a) is ahead of (h) and of (c) by more than the larger spread of the two sides.  These calls are latency-bound;
run-to-run noise is what a smaller difference cannot be told from.  Nothing is claimed as a share of peak.

Every row runs in a child process of its own under its own time limit; after a row that fails or runs out of time nothing more is
started.  --profile-row NAME runs the row's (a) three times after one warm-up, for a per-kernel trace from outside.

    python tools/bench_distance_loss.py [--repeats 7] [--out profiles/distance_loss_bench.txt]
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

from bench_distance import alternate, fmt  # noqa: E402

ROWS = ("boundary_2d", "hausdorff_2d", "boundary_3d", "hausdorff_3d", "boundary_2d_maps")
ROW_LIMIT_S = {"boundary_2d": 240, "hausdorff_2d": 300, "boundary_3d": 300, "hausdorff_3d": 420, "boundary_2d_maps": 240}
SHAPES = {"2d": (8, 4, (512, 512)), "3d": (2, 3, (128, 128, 128))}


def make_inputs(row, dev):
    from bench_metrics import blob_labels

    B, C, spatial = SHAPES[row.split("_")[1]]
    g = torch.Generator().manual_seed(3)
    x = (2.0 * torch.randn((B, C) + spatial, generator=g)).to(dev)
    labels = torch.stack([blob_labels(spatial, C, 20 + b, dev) for b in range(B)]).to(torch.int64)
    return x, labels, C, len(spatial)


def torch_tail(kind, x, phi_t, phi_p, onehot):
    """the loss from maps [B, C, *spatial] as torch ops: softmax, multiply, mean"""
    p = torch.softmax(x, dim=1)
    if kind == "boundary":
        return (p * phi_t).mean()
    return ((p - onehot) ** 2 * (phi_p ** 2 + phi_t ** 2)).mean()


def scipy_signed(objects, edt):
    """float32 signed maps of the boolean numpy array [B, C, *spatial], entry by entry; 0 where an entry has no boundary"""
    out = np.zeros(objects.shape, np.float32)
    for b in range(objects.shape[0]):
        for c in range(objects.shape[1]):
            m = objects[b, c]
            if m.any() and not m.all():
                out[b, c] = edt(~m) - edt(m)
    return out


def run_row(row, args):
    """one row in this process; prints its lines and a last line of JSON for the parent"""
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd import losses
    from pytorch_toolbelt_amd.utils import class_distance_maps, distance_transform

    dev = torch.device("cuda:0")
    kind = row.split("_")[0]
    x, labels, C, dims = make_inputs(row, dev)
    x.requires_grad_(True)
    given = class_distance_maps(labels, num_classes=C, dims=dims, squared=True) if row.endswith("_maps") else None
    given_f = class_distance_maps(labels, num_classes=C, dims=dims) if given is not None else None
    crit = losses.BoundaryLoss("multiclass") if kind == "boundary" else losses.HausdorffDTLoss("multiclass")
    classes = torch.arange(C, device=dev).reshape((1, C) + (1,) * dims)
    lines, values = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def finish(name, loss):
        x.grad = None
        loss.backward()
        values[name] = loss.detach()
        return x.grad

    def side_a():
        return finish("a", crit(x, labels, dist_maps=given))

    def finite(t):
        return torch.where(torch.isfinite(t), t, torch.zeros_like(t))

    def side_c():
        onehot = (labels.unsqueeze(1) == classes).float()
        phi_t = finite(torch.stack([distance_transform(labels, foreground=c, signed=True, dims=dims) for c in range(C)], dim=1))
        phi_p = None
        if kind == "hausdorff":
            hard = (torch.softmax(x.detach(), dim=1) > 0.5).to(torch.uint8)
            phi_p = finite(torch.stack([distance_transform(hard[:, c], foreground=1, signed=True, dims=dims) for c in range(C)], dim=1))
        return finish("c", torch_tail(kind, x, phi_t, phi_p, onehot))

    def side_h(edt):
        onehot = labels.unsqueeze(1) == classes
        phi_t = torch.from_numpy(scipy_signed(onehot.cpu().numpy(), edt)).to(dev)
        phi_p = None
        if kind == "hausdorff":
            hard = torch.softmax(x.detach(), dim=1) > 0.5
            phi_p = torch.from_numpy(scipy_signed(hard.cpu().numpy(), edt)).to(dev)
        return finish("h", torch_tail(kind, x, phi_t, phi_p, onehot.float()))

    def side_t():
        return finish("t", torch_tail(kind, x, finite(given_f), None, None))

    say(f"{row}: logits {list(x.shape)} fp32, labels {list(labels.shape)} int64, {C} classes" + (", dist_maps= given (int32 squared)" if given is not None else ""))
    sides = {"a": side_a, "c": side_c}
    if given is not None:
        sides["t"] = side_t
    try:
        from scipy.ndimage import distance_transform_edt as edt

        sides["h"] = lambda: side_h(edt)
    except ImportError:
        say("  (h) left out: scipy is not installed on this machine")
    grads = {k: f().clone() for k, f in sides.items()}            # (the warm-up of every side is the call whose result is compared)
    torch.cuda.synchronize()
    ref = float(values["a"])
    for k in sides:
        if k != "a":
            gd = float((grads[k] - grads["a"]).abs().max() / grads["a"].abs().max())
            say(f"  ({k}) against (a): loss {float(values[k]):.7g} against {ref:.7g} (relative {abs(float(values[k]) - ref) / max(abs(ref), 1e-30):.1e}), "
                f"largest gradient difference / largest gradient {gd:.1e}")
    del grads
    tm = alternate(sides, args.repeats)
    names = {"a": f"{type(crit).__name__} forward + backward", "h": "D2H + scipy per sample and class + H2D + torch ops", "c": "distance_transform per class + torch ops",
             "t": "torch ops on the given maps"}
    for k, t in tm.items():
        say(f"  ({k}) {names[k]:52s} {fmt(t)}")
    result = {"row": row, "median_a": float(np.median(tm["a"])), "bar": None}
    met = []
    for k in ("h", "c"):
        if k not in tm:
            continue
        gap = float(np.median(tm[k]) - np.median(tm["a"]))
        spread = float(max(np.ptp(tm["a"]), np.ptp(tm[k])))
        ok = gap > spread
        met.append(ok)
        text = f"({k}) - (a) = {gap * 1e3:.3f} ms, larger spread {spread * 1e3:.3f} ms: (a) is {'ahead' if ok else 'NOT ahead'} of ({k}) by more than the spread (({k}) / (a) = {np.median(tm[k]) / np.median(tm['a']):.1f})"
        say("  " + (text if ok else f"**{text}**"))
    if "t" in tm:
        say(f"  (t) / (a) = {np.median(tm['t']) / np.median(tm['a']):.2f}   [reported, not barred]")
    if len(met) == 2:
        result["bar"] = all(met)
    result["lines"] = lines
    print("RESULT " + json.dumps(result), flush=True)


def profile_row(row, args):
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd import losses
    from pytorch_toolbelt_amd.utils import class_distance_maps

    dev = torch.device("cuda:0")
    kind = row.split("_")[0]
    x, labels, C, dims = make_inputs(row, dev)
    x.requires_grad_(True)
    given = class_distance_maps(labels, num_classes=C, dims=dims, squared=True) if row.endswith("_maps") else None
    crit = losses.BoundaryLoss("multiclass") if kind == "boundary" else losses.HausdorffDTLoss("multiclass")
    for _ in range(4):                       # (one warm-up and three calls; the per-kernel SHARES are what is read from the trace)
        x.grad = None
        crit(x, labels, dist_maps=given).backward()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", help="(internal) run one row in this process")
    ap.add_argument("--profile-row", choices=ROWS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_loss_bench.txt"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("bench_distance_loss: at least 7 repeats")
    if not torch.cuda.is_available():
        sys.exit("bench_distance_loss: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    if args.profile_row:
        return profile_row(args.profile_row, args)
    if args.row:
        return run_row(args.row, args)
    lines = [f"distance-map losses on {torch.cuda.get_device_name(0)}; forward + backward, {args.repeats} alternating repeats (order reversed every round) after 1 "
             "warm-up run of every side; host clock around device-synchronised calls; every row in a process of its own under its own time limit"]
    print(lines[0], flush=True)
    results, failed = {}, None
    rows = args.rows.split(",")
    for row in rows:
        cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--repeats", str(args.repeats)]
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
    have = [r for r in rows if r in results]
    if failed or len(have) < len(ROWS):
        lines.append(f"THE BAR: **not established: of the rows {ROWS} only {tuple(have)} ran here**" + (f"; on those: {[(r, results[r]['bar']) for r in have]}" if have else ""))
    elif any(results[r]["bar"] is None for r in ROWS):
        lines.append("THE BAR: **not established: scipy is not installed on this machine**")
    else:
        lines.append("THE BAR (on every row the fused path is ahead of the host route and of the composition on the device by more than the larger spread): "
                     + ("met" if all(results[r]["bar"] for r in ROWS) else "**NOT met**") + f" {[(r, results[r]['bar']) for r in ROWS]}")
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
