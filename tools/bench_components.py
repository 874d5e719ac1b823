#!/usr/bin/env python3
"""Benchmark of the connected-component kernels on one MI355X (utils/components.py, csrc/ptb_components.hip).

Inputs, seeded and generated here: 5000 x 5000 uint8 maps -- a 4-class blob label map as merge_crop(argmax=True, dtype=torch.uint8)
leaves it, 50 % binary noise, all ones (ONE component of 25 million positions: every area lands on one address), a serpentine (one
component whose path is H * W / 2 long) -- and one 512^3 4-class blob volume under connectivity 6 and 26.

Timed, each call from its start to a device synchronise behind its last piece of work, after a warm-up of every side, in rounds that
alternate between the sides (the order inside a round turns over every round):
  (a) connected_components                      -- nothing read back
  (r) remove_small_components(min_area=64)      -- no scan, nothing read back
  (h) the host route: D2H + scipy.ndimage.label (per class for the multi-class map, offsets added) + H2D of the int32 result.
      Without scipy on this machine the side is left out and the file says so.  5000 x 5000 rows only.
  (t) the torch-op chain people use on the device today: labels = position + 1, then 3 x 3 max-pooling within each class iterated to
      convergence (checked every 32 iterations; float64, because float32 cannot hold 25 million distinct labels).  Blob map only: it
      needs as many passes as the longest path inside a component, which on the serpentine is 12.5 million.
Reported per row: median and spread (max - min) of the repeats, the bytes the kernels move (a model: see bytes_moved) as a share of the
copy rate measured in this process -- no claim is made about it: the workload is latency- and atomic-bound -- and whether the sides agree.
THE BAR: on the blob map and on the noise map (a) beats (h) by more than the larger spread of the two; on the blob map (a) also
beats (t) by more than the larger spread.  All-ones, serpentine, volume and every (r) row are reported only.

Every row runs in a child process of its own under its own time limit; after a row that fails or runs out of time nothing more is
started.  --profile-map NAME runs remove_small_components once on that map after one warm-up, for a per-kernel trace from outside.

    python tools/bench_components.py [--repeats 7] [--edge 5000] [--cube 512] [--out profiles/components_bench.txt]
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

ROWS = ("blobs", "noise", "ones", "serpentine", "volume6", "volume26")
ROW_LIMIT_S = {"blobs": 420, "noise": 150, "ones": 150, "serpentine": 150, "volume6": 200, "volume26": 200}
MIN_AREA = 64


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def alternate(sides, repeats, warmup=1):
    for _ in range(warmup):
        for fn in sides.values():
            once(fn)
    times = {k: [] for k in sides}
    order = list(sides)
    for r in range(repeats):
        for k in (order if r % 2 == 0 else order[::-1]):
            times[k].append(once(sides[k]))
    return {k: np.array(v) for k, v in times.items()}


def make_map(row, edge, cube, dev):
    from bench_metrics import blob_labels

    if row == "blobs":
        return blob_labels((edge, edge), 4, 0, dev), 2, 8
    if row == "noise":
        g = torch.Generator().manual_seed(1)
        return torch.randint(0, 2, (edge, edge), generator=g, dtype=torch.uint8).to(dev), 2, 8
    if row == "ones":
        return torch.ones((edge, edge), dtype=torch.uint8, device=dev), 2, 8
    if row == "serpentine":
        a = torch.zeros((edge, edge), dtype=torch.uint8, device=dev)
        a[0::2] = 1
        ys = torch.arange(1, edge - 1, 2, device=dev)
        a[ys, torch.where(torch.arange(ys.numel(), device=dev) % 2 == 0, edge - 1, 0)] = 1
        return a, 2, 8
    return blob_labels((cube,) * 3, 4, 2, dev), 3, 6 if row == "volume6" else 26


def copy_rate(dev):
    """bytes per second (read + written) of a 256 MB device-to-device copy, the median of 5"""
    src = torch.empty(64 << 20, dtype=torch.int32, device=dev)
    dst = torch.empty_like(src)
    once(lambda: dst.copy_(src))
    t = np.median([once(lambda: dst.copy_(src)) for _ in range(5)])
    return 2 * src.numel() * 4 / t


def bytes_moved(n, elem, remove):
    """a model of the traffic of one call over n positions, seams and scan left out (a few per cent): the map read once and the int32
    parent map written (local), parents read and roots written (flatten); then, labelling: roots read (rank), roots read, ranks gathered
    and cc written (relabel); remove_small: the area map zeroed, roots read (area), map and roots read, areas gathered, map written"""
    return n * (elem + 4 + 8 + (4 + 12 if not remove else 4 + 4 + elem + 8 + elem))


def chain(labels):
    """max-pool label propagation within each class, iterated to convergence (checked every 32 iterations)"""
    import torch.nn.functional as F

    H, W = labels.shape
    classes = [c for c in range(1, 4)]
    mask = torch.stack([labels == c for c in classes])[None]
    idx = torch.arange(1, H * W + 1, device=labels.device, dtype=torch.float64).view(1, 1, H, W)
    lab = idx * mask
    passes = 0
    while True:
        before = lab
        for _ in range(32):
            lab = F.max_pool2d(lab, 3, stride=1, padding=1) * mask
        passes += 32
        if torch.equal(before, lab):
            return lab, passes


def host_route(labels, scipy_label, structure, dev):
    h = labels.cpu().numpy()
    out = np.zeros(h.shape, np.int32)
    offset = 0
    for c in np.unique(h[h != 0]) if h.max() > 1 else (1,):
        lab, n = scipy_label(h == c, structure=structure)
        out[lab > 0] = lab[lab > 0] + offset
        offset += n
    return torch.from_numpy(out).to(dev), offset


def fmt(t):
    return f"{np.median(t) * 1e3:10.3f} ms (spread {(t.max() - t.min()) * 1e3:8.3f} ms)"


def run_row(row, args):
    """one row in this process; prints its lines and a last line of JSON for the parent"""
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import connected_components, remove_small_components

    dev = torch.device("cuda:0")
    labels, dims, conn = make_map(row, args.edge, args.cube, dev)
    rate = copy_rate(dev)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def side_a():
        return connected_components(labels, connectivity=conn, dims=dims)

    def side_r():
        return remove_small_components(labels, MIN_AREA, connectivity=conn, dims=dims)

    cc, count = side_a()
    n = labels.numel()
    say(f"{row}: {list(labels.shape)} uint8, connectivity {conn}: {int(count)} components, {int((cc != 0).sum())} of {n} positions in one; "
        f"remove_small(min_area={MIN_AREA}) changes {int((side_r() != labels).sum())} positions; copy rate here {rate / 1e12:.2f} TB/s")
    assert int(count) >= 0
    sides = {"a": side_a, "r": side_r}
    scipy_label = None
    if dims == 2:
        try:
            from scipy import ndimage

            scipy_label = ndimage.label
            structure = ndimage.generate_binary_structure(2, 2)
        except ImportError:
            say("  (h) left out: scipy is not installed on this machine")
    if scipy_label is not None:
        sides["h"] = lambda: host_route(labels, scipy_label, structure, dev)
        _, n_host = sides["h"]()
        say(f"  (h) finds {n_host} components: {'equal' if n_host == int(count) else '**DIFFERENT**'}")
    if row == "blobs":
        sides["t"] = lambda: chain(labels)
        lab, passes = sides["t"]()
        n_chain = sum(int(torch.unique(lab[0, k]).numel()) - 1 for k in range(lab.shape[1]))
        say(f"  (t) converges after {passes} passes and finds {n_chain} components: {'equal' if n_chain == int(count) else '**DIFFERENT**'}")
        del lab
    elif row == "serpentine":
        say(f"  (t) not run: the component's path is {n // 2} positions long, so the chain needs that many full-image passes")
    tm = alternate(sides, args.repeats)
    names = {"a": "connected_components", "r": f"remove_small_components({MIN_AREA})", "h": "D2H + scipy.ndimage.label + H2D", "t": "max-pool chain on device"}
    for k, t in tm.items():
        extra = ""
        if k in "ar":
            b = bytes_moved(n, 1, k == "r")
            extra = f"   {b / 1e6:8.0f} MB moved = {100 * b / np.median(t) / rate:5.1f} % of the copy rate"
        say(f"  ({k}) {names[k]:34s} {fmt(t)}{extra}")
    result = {"row": row, "median_a": float(np.median(tm["a"])), "median_r": float(np.median(tm["r"])), "bar": {}}
    for k in ("h", "t"):
        if k in tm and row in ("blobs", "noise"):
            gap = float(np.median(tm[k]) - np.median(tm["a"]))
            spread = float(max(np.ptp(tm["a"]), np.ptp(tm[k])))
            met = gap > spread
            text = f"({k}) - (a) = {gap * 1e3:.3f} ms, larger spread {spread * 1e3:.3f} ms: the bar is {'met' if met else 'NOT met'} (({k}) / (a) = {np.median(tm[k]) / np.median(tm['a']):.1f})"
            say("  " + (text if met else f"**{text}**"))
            result["bar"][k] = met
    result["lines"] = lines
    print("RESULT " + json.dumps(result), flush=True)


def profile_map(row, args):
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd.utils import remove_small_components

    dev = torch.device("cuda:0")
    labels, dims, conn = make_map(row, args.edge, args.cube, dev)
    for _ in range(2):                       # (the trace holds both; the per-kernel SHARES are what is read from it)
        remove_small_components(labels, MIN_AREA, connectivity=conn, dims=dims)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--edge", type=int, default=5000)
    ap.add_argument("--cube", type=int, default=512)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", help="(internal) run one row in this process")
    ap.add_argument("--profile-map", choices=ROWS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.txt"))
    args = ap.parse_args()
    if args.repeats < 7:
        sys.exit("bench_components: at least 7 repeats")
    if not torch.cuda.is_available():
        sys.exit("bench_components: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    if args.profile_map:
        return profile_map(args.profile_map, args)
    if args.row:
        return run_row(args.row, args)
    lines = [f"connected components on {torch.cuda.get_device_name(0)}; {args.repeats} alternating repeats (order reversed every round) after 1 warm-up run "
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
        for k in ("ones", "serpentine"):
            if k in results:
                for side in "ar":
                    lines.append(f"{k} / blobs, ({side}): {results[k]['median_' + side] / results['blobs']['median_' + side]:.2f}")
    bars = [m for r in results.values() for m in r["bar"].values()]
    need = sum(1 for r in ("blobs", "noise") if r in results)
    if failed or need < 2:
        lines.append("THE BAR: **not established: a required row is missing**")
    elif any("h" not in results[r]["bar"] for r in ("blobs", "noise")):
        lines.append("THE BAR: **not established against the host route: scipy is not installed on this machine**; against the max-pool chain on the blob map: "
                     + ("met" if results["blobs"]["bar"].get("t") else "**NOT met**"))
    else:
        lines.append("THE BAR ((a) beats the host route on the blob and noise maps and the max-pool chain on the blob map by more than the spread): "
                     + ("met" if bars and all(bars) else "**NOT met**") + f" {[(r, results[r]['bar']) for r in ('blobs', 'noise')]}")
    print("\n".join(lines[-4:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
