#!/usr/bin/env python3
"""The headline loop on channels-last model outputs (a model in torch.channels_last: what MIOpen's convolutions want under AMP):
5000 x 5000, 512-pixel tiles every 256, d4, C = 4, batches of 8 tiles; fp32 and bf16 outputs; three loops --

    explicit   TileMerger(crops=, defer=True) + integrate_batch_deaugment(y, crops, "d4", "mean")
    literal    a new TileMerger per image + integrate_batch(tta.d4_image_deaugment(y), crops)   (self-planned from the second image on)
    no_tta     TileMerger(crops=, defer=True) + integrate_batch(y, crops)

each timed (a) on this tree with channels-last batches, (b) on this tree with the same values dense, and -- with --parent-root, a
checkout of the parent commit with its library built -- (c) with the channels-last batches on that tree, which copies every batch to
NCHW first.  Every (tree, layout) runs in a process of its own, the processes alternate and the whole round is repeated, so the
spread printed per row is the run-to-run spread of the same code on the same box.

    python tools/bench_channels_last.py --parent-root /path/to/parent/checkout --out profiles/channels_last_bench
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ("float32", "bfloat16")
LOOPS = ("explicit", "literal", "no_tta")


def worker(root, layout, warmup, images):
    """One process: every (dtype, loop) row for one tree and one layout; prints one JSON line per row."""
    sys.path.insert(0, root)
    import torch

    from pytorch_toolbelt_amd.inference import tta
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer, TileMerger

    dev = torch.device("cuda:0")
    slicer = ImageSlicer((5000, 5000, 3), 512, 256, weight="pyramid")
    crops = slicer.crops
    n, C, bs = len(crops), 4, 8
    pc = [crops[b0:b0 + bs] for b0 in range(0, n, bs)]
    for dt_name in DTYPES:
        dt = getattr(torch, dt_name)
        for loop in LOOPS:
            V = 1 if loop == "no_tta" else 8
            g = torch.Generator(device=dev).manual_seed(0)
            outs = []
            for b0 in range(0, n, bs):
                y = torch.randn((V * min(bs, n - b0), C, 512, 512), device=dev, generator=g).to(dt)
                outs.append(y.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else y)
            fixed = TileMerger(slicer.target_shape, C, slicer.weight, device=dev, crops=crops, defer=True) if loop != "literal" else None

            def image():
                if loop == "literal":
                    m = TileMerger(slicer.target_shape, C, slicer.weight, device=dev)
                    for t, c in zip(outs, pc):
                        m.integrate_batch(tta.d4_image_deaugment(t), c)
                    return m.merge()
                fixed.reset()
                if loop == "explicit":
                    for t, c in zip(outs, pc):
                        fixed.integrate_batch_deaugment(t, c, group="d4", reduction="mean")
                else:
                    for t, c in zip(outs, pc):
                        fixed.integrate_batch(t, c)
                return fixed.merge()

            for _ in range(warmup):
                out = image()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(images):
                out = image()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / images
            read = V * n * C * 512 * 512 * outs[0].element_size()
            written = out.numel() * 4
            print(json.dumps({"dtype": dt_name, "loop": loop, "layout": layout, "ms": ms, "bytes_read": read, "bytes": read + written,
                              "checksum": float(out.double().nan_to_num().sum())}), flush=True)
            del outs, fixed, out
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built: variant (c)")
    ap.add_argument("--repeats", type=int, default=3, help="rounds over the variants (alternating processes)")
    ap.add_argument("--warmup", type=int, default=10, help="untimed images per row")
    ap.add_argument("--images", type=int, default=20, help="timed images per row")
    ap.add_argument("--out", default=None, help="write OUT.json and OUT.txt")
    ap.add_argument("--worker", nargs=2, metavar=("ROOT", "LAYOUT"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker[0], args.worker[1], args.warmup, args.images)

    variants = []
    if args.parent_root:
        variants.append(("parent_channels_last", os.path.abspath(args.parent_root), "channels_last"))
    variants += [("channels_last", HERE, "channels_last"), ("dense", HERE, "dense")]
    runs = {name: {} for name, _r, _l in variants}       # variant -> (dtype, loop) -> [row per repeat]
    for rep in range(args.repeats):
        for name, root, layout in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, layout, "--warmup", str(args.warmup), "--images", str(args.images)]
            env = dict(os.environ)
            env.pop("PTB_HIP_LIB", None)
            res = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=root)
            if res.returncode != 0:
                sys.stderr.write(res.stderr[-4000:])
                raise SystemExit(f"{name}: worker failed with status {res.returncode}")
            for line in res.stdout.splitlines():
                if line.startswith("{"):
                    row = json.loads(line)
                    runs[name].setdefault((row["dtype"], row["loop"]), []).append(row)
            print(f"[round {rep + 1}/{args.repeats}] {name} done", file=sys.stderr, flush=True)

    rows, lines = [], []
    lines.append("5000 x 5000, 512-pixel tiles every 256, d4 (no_tta: one view), C = 4, batches of 8 tiles; ms per image, median of "
                 f"{args.repeats} processes ({args.images} timed images each); spread = (max - min) / median over the processes")
    for dt in DTYPES:
        for loop in LOOPS:
            rec = {"dtype": dt, "loop": loop}
            for name in runs:
                ms = [r["ms"] for r in runs[name].get((dt, loop), [])]
                if not ms:
                    continue
                med = statistics.median(ms)
                rec[name] = {"ms": med, "runs_ms": ms, "spread": (max(ms) - min(ms)) / med}
                rec["bytes_read"] = runs[name][(dt, loop)][0]["bytes_read"]
                rec.setdefault("checksums", {})[name] = runs[name][(dt, loop)][0]["checksum"]
            cl, dense, parent = rec.get("channels_last"), rec.get("dense"), rec.get("parent_channels_last")
            assert len(set(rec["checksums"].values())) == 1, f"{dt} {loop}: the variants disagree: {rec['checksums']}"
            rec["channels_last_over_dense"] = cl["ms"] / dense["ms"]
            rec["fraction_of_8TBs_bytes_read"] = rec["bytes_read"] / (cl["ms"] * 1e-3) / 8e12
            text = (f"{dt:9s} {loop:9s} channels-last {cl['ms']:7.3f} ms (spread {cl['spread'] * 100:4.1f} %)   dense {dense['ms']:7.3f} ms "
                    f"(spread {dense['spread'] * 100:4.1f} %)   channels-last / dense {rec['channels_last_over_dense']:5.2f}   "
                    f"{rec['bytes_read'] / 1e9:6.2f} GB read = {rec['fraction_of_8TBs_bytes_read'] * 100:5.1f} % of 8 TB/s")
            if parent:
                rec["parent_over_channels_last"] = parent["ms"] / cl["ms"]
                rec["faster_than_parent_beyond_its_spread"] = bool(parent["ms"] - cl["ms"] > parent["spread"] * parent["ms"])
                text += (f"   parent (copies) {parent['ms']:7.3f} ms (spread {parent['spread'] * 100:4.1f} %)   parent / channels-last "
                         f"{rec['parent_over_channels_last']:5.2f}   faster beyond the parent's spread: {rec['faster_than_parent_beyond_its_spread']}")
            rows.append(rec)
            lines.append(text)
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump({"rows": rows}, open(args.out + ".json", "w"), indent=1)
        open(args.out + ".txt", "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
