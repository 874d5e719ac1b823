#!/usr/bin/env python3
"""Benchmark of the dims=3 skeleton kernels on one MI355X (utils/skeleton.py, csrc/ptb_skeleton3d.hip).

Rows, seeded and generated here, outside the timed region:
  blobs128, blobs256     a bool volume of smooth blobs (a gaussian-filtered seeded random field above its median): skeletonize(v, dims=3)
  vessels128, vessels256 thin tubes: seeded random walks dilated to a radius of 2
  cldice128              centerline_dice(dims=3) of a 3-class blob volume and the same volume shifted by (2, 3, 5)

Timed, each call from its start to a device synchronise behind its last piece of work, after a warm-up of every side, in rounds that
alternate between the sides:
  (a) the device call; its iteration count and the launches of the thinning kernel are recorded (one native call with took[2])
  (h) D2H + THE LIBRARY'S OWN CPU FORM + H2D -- the only other implementation of this definition; at 128^3 only (--host-repeats samples),
      and its result is compared with (a) bit for bit
Every row runs in a child process of its own under its own time limit; after a row that fails or runs out of time nothing more is
started.  The file is rewritten after every row; everything from the line that starts with KEPT_MARKER on is kept from the existing file
(the A/B of the brick, the halo and the passes per launch: build the library with e.g. -DPTB_THIN3D_OZ=32 -DPTB_THIN3D_OY=32
-DPTB_THIN3D_PASSES=2 into a directory of its own and run  PTB_HIP_LIB=.../libptb_hip.so python tools/bench_skeleton3d.py --ab-row).

    python tools/bench_skeleton3d.py [--repeats 7] [--host-repeats 3] [--out profiles/skeleton3d_bench.txt]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_distance import fmt, once  # noqa: E402

ROWS = ("blobs128", "vessels128", "cldice128", "blobs256", "vessels256")
ROW_LIMIT_S = {"blobs128": 400, "vessels128": 300, "cldice128": 600, "blobs256": 300, "vessels256": 300}
KEPT_MARKER = "==== kept by tools/bench_skeleton3d.py"


def make_volume(kind, edge, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "blobs":
        f = ndimage.gaussian_filter(rng.random((edge, edge, edge), dtype=np.float32), edge / 16)
        return f > np.median(f)
    v = np.zeros((edge, edge, edge), bool)
    for _ in range(edge // 4):                              # random walks with a slowly turning direction
        p, d = rng.random(3) * edge, rng.normal(size=3)
        for _ in range(2 * edge):
            d = d + 0.3 * rng.normal(size=3)
            d /= np.linalg.norm(d)
            p = p + d
            if (p < 0).any() or (p >= edge).any():
                break
            v[tuple(p.astype(int))] = True
    return ndimage.binary_dilation(v, ndimage.generate_binary_structure(3, 1), 2)


def device_call(x):
    """skeletonize(x, dims=3) as the public function calls the library, with both words of took"""
    from pytorch_toolbelt_amd import _native as N
    from pytorch_toolbelt_amd.utils import _maps as M

    D, H, W = x.shape
    res = torch.empty(x.shape, dtype=torch.bool, device=x.device)
    ws, nbytes = M.workspace(N.load().ptb_skeleton3d_plan, "bench", x.device, 1, D, H, W)
    took = (ctypes.c_int * 2)(0, 0)
    N.check(N.launch("ptb_skeleton3d", x.device, x.data_ptr(), 1, 1, D, H, W, 1, 0, -1, res.data_ptr(), took, ws.data_ptr(), nbytes, raw=True), "bench")
    return res, took[0], took[1]


def run_row(row, args):
    import __graft_entry__ as g

    if not os.environ.get("PTB_HIP_LIB"):
        g.build()
    from pytorch_toolbelt_amd.utils import centerline_dice, skeletonize

    dev = torch.device("cuda:0")
    kind, edge = row.rstrip("0123456789"), int(row[-3:])
    lines = []
    if kind == "cldice":
        labels = make_volume("blobs", edge) * np.random.default_rng(1).integers(1, 4, (edge,) * 3).astype(np.uint8)
        pred, truth = torch.from_numpy(labels).to(dev), torch.from_numpy(np.roll(labels, (2, 3, 5), (0, 1, 2))).to(dev)
        side_a = lambda: centerline_dice(pred, truth, labels=[1, 2, 3], dims=3)["counts"]
        side_h = lambda: centerline_dice(pred.cpu(), truth.cpu(), labels=[1, 2, 3], dims=3)["counts"].to(dev)
        got = side_a()
        head = f"{row}: centerline_dice(dims=3), 3 classes, [{edge}]^3 uint8; counts of class 1: {got[0].tolist()}"
    else:
        x = torch.from_numpy(make_volume(kind, edge)).to(dev)
        side_a = lambda: skeletonize(x, dims=3)
        side_h = lambda: skeletonize(x.cpu(), dims=3).to(dev)
        got, iterations, launches = device_call(x)
        assert torch.equal(got, side_a())
        head = (f"{row}: skeletonize(dims=3), [{edge}]^3 bool: {int(x.sum())} of {x.numel()} positions set, {int(got.sum())} in the skeleton after {iterations} iterations, "
                f"{launches} launches of the thinning kernel")
    lines.append(head)
    times = {"a": [], "h": []}
    host = edge <= 128
    if host:
        t = once(lambda: lines.append("  (a) " + ("equals" if torch.equal(side_h(), got) else "**DIFFERS FROM**") + " (h) bit for bit"))
        if args.host_repeats == 0:
            times["h"].append(t)
    once(side_a)
    for r in range(args.repeats):
        for k in ("a", "h") if r % 2 == 0 else ("h", "a"):
            if k == "a" or (host and r < args.host_repeats):
                times[k].append(once(side_a if k == "a" else side_h))
    lines.append(f"  (a) the device call                                  {fmt(np.array(times['a']))}  [{len(times['a'])} samples]")
    if times["h"]:
        th = np.array(times["h"])
        lines.append(f"  (h) D2H + the library's CPU form + H2D               {fmt(th)}  [{len(th)} samples]   (h) / (a) = {np.median(th) / np.median(times['a']):.1f}")
    else:
        lines.append("  (h) not run at this size")
    print("\n".join(lines), flush=True)
    print("RESULT " + json.dumps({"lines": lines}), flush=True)


def ab_row(args):
    """one line: the blob row with the library that is loaded (PTB_HIP_LIB)"""
    from pytorch_toolbelt_amd import _native as N

    geometry = (ctypes.c_int * 5)()
    N.load().ptb_thin3d_geometry(geometry)
    for edge in (128, 256):
        x = torch.from_numpy(make_volume("blobs", edge)).to("cuda:0")
        got, iterations, launches = device_call(x)
        once(lambda: device_call(x))
        t = np.array([once(lambda: device_call(x)) for _ in range(args.repeats)])
        print(f"brick {geometry[0]} x {geometry[1]} x {geometry[2]}, halo {geometry[3]}, {geometry[4]} pass(es) a launch: blobs{edge}, {iterations} iterations, {launches} launches, "
              f"{int(got.sum())} skeleton positions: {fmt(t)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--rows", default=",".join(ROWS))
    ap.add_argument("--row", help="(internal) run one row in this process")
    ap.add_argument("--ab-row", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skeleton3d_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_skeleton3d: no GPU found (this benchmark measures the MI355X and has no CPU mode)")
    if args.ab_row:
        return ab_row(args)
    if args.row:
        return run_row(args.row, args)
    lines = [f"skeletonize(dims=3) and centerline_dice(dims=3) on {torch.cuda.get_device_name(0)}; {args.repeats} alternating repeats (the host side (h) in {args.host_repeats} of them, "
             "at 128^3 only) after 1 warm-up run of every side; host clock around device-synchronised calls; every row in a process of its own under its own time limit"]
    try:
        old = open(args.out).read().splitlines()
    except OSError:
        old = []
    at = [i for i, ln in enumerate(old) if ln.startswith(KEPT_MARKER)]
    kept = old[at[0]:] if at else []
    status = 0
    for row in args.rows.split(","):
        shown = len(lines)
        cmd = [sys.executable, os.path.abspath(__file__), "--row", row, "--repeats", str(args.repeats), "--host-repeats", str(args.host_repeats)]
        try:
            child = subprocess.run(cmd, capture_output=True, text=True, timeout=ROW_LIMIT_S[row])
        except subprocess.TimeoutExpired:
            lines.append(f"**{row}: no result within its time limit of {ROW_LIMIT_S[row]} s; nothing more was started**")
            status = 1
        else:
            res = [ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")]
            if child.returncode != 0 or not res:
                lines.append(f"**{row}: exit status {child.returncode}; nothing more was started**\n" + child.stderr[-2000:])
                status = 1
            else:
                lines += json.loads(res[-1][7:])["lines"]
        print("\n".join(lines[shown:]), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines + ([""] + kept if kept else [])) + "\n")
        if status:
            break
    return status


if __name__ == "__main__":
    sys.exit(main())
