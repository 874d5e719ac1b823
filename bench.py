#!/usr/bin/env python3
"""Headline benchmark: megapixels/s of the tiled + d4-TTA merge on 5000x5000 (BASELINE.json configs[1]).

One *step* = one full pass of the hot path over one 5000x5000x3 image: 361 tiles (512/256, pyramid window) whose
8 d4-view model outputs (C=4, fp32, 12.1 GB) are already resident in HBM -> `integrate_batch_deaugment` (fused de-augment +
mean + weighted blend) in batches of 8 tiles -> `merge()` (image / norm_mask).  The model forward is excluded (the
config's "dummy UNet" only produces these tensors).  Every step starts from a `reset()` merger and ends with the merged
[C, 5120, 5120] map in HBM.

Default merger: `TileMerger(..., crops=tiler.crops, defer=True)`.  The crop list is known before the first batch (the
README loop has it), so the normaliser `norm_mask` -- which depends only on the crop list and the window (not
compulsory traffic) -- is precomputed, and the merger keeps references to the batches it is handed (they stay resident
and unmodified here) and merges every group of 1024 rows of the image (four 256-row bands between tile edges; `--defer-rows`)
with ONE launch as soon as its last tile has arrived: 5 launches per image that read every model output once and write the
merged map once; no accumulator in HBM.  A/B switches:
`--no-defer` (planned, incremental: 46 accumulate launches, every block divided by the normaliser in the launch that
brings its last tile), `--unplanned` (no crop list: accumulate kernels + lazily built normaliser + separate division
pass), `--memset-accumulators` (kernel-maintained normaliser, memset accumulators: the reference's literal data flow).
All four produce bit-identical results (tests/test_tiles_gpu.py).

`value` is measured on the model-output pool exactly as torch's allocator first hands it out: a ramp until the step time has
settled, the W warm-up steps, and EXACTLY K timed steps `--repeats` times (value = the median run).  Which device memory backs
the 12 GB decides up to 10-15 % of the loop's speed on some boxes (tools/placement_map.py); what a process that owns its buffers
could gain by choosing among `--placement-tries` candidate pools is measured AFTER the headline (with `--full`) and reported
separately as `config.best_placement` (never `value`).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A plain run does only what the headline needs: set-up, ramp and warm-up, the timed steps, `--dump-outputs`, the JSON line.
`--full` adds everything else the benchmark measures or checks, all of it after the headline was timed: the timed output against
the plain merger (`config.parity`, a mismatch fails the run), the secondary timings of the API variants (`config.variants`), the
roofline block with this box's read ceiling, the placement search (`config.best_placement`), the other BASELINE configs and the
end-to-end loops on this GPU (`config.secondary`) and the CPU baselines (`cpu_baseline`); for N > 1 the parity of every rank's band
before timing and the exchange's cost (`config.sharded`).  `--no-variants`, `--no-secondary`, `--no-cpu-baseline` and
`--placement-tries 1` leave single parts of it out.

`--dump-outputs DIR` (one GPU) writes what the last timed step returned -- the merged map, as a fixed seeded sample of its values --
to DIR/merged_sample.npy, so that two builds run with the same arguments can be compared output for output.

N > 1 runs one rank per GPU over RCCL; started without WORLD_SIZE in the environment, `python bench.py --gpus N` launches itself
under torch.distributed.run (127.0.0.1, a free port).  With `--full`, before anything is timed every rank checks the rows it owns
against the SINGLE-DEVICE merge of the same (per-tile seeded) model outputs; the JSON line carries `config.sharded.parity_max_abs_diff`
and `rccl_ranks` (ranks whose exchange is the library's own RCCL communicator), and a parity failure fails the run.  The 361 tiles of ONE image are sharded over the
ranks as contiguous tile ranges (45 / 46 tiles each at N = 8), neighbouring ranks exchange their 256-row halo rectangles
point-to-point over xGMI (one ncclGroup per image on the library's own communicator) and every rank merges its own band (strong
scaling: total work per step is fixed).  Steps are pipelined (`merge_async`): image i's exchange runs beside image i+1's kernels;
the K timed steps are K whole images, the last one completed inside the timed region.  `config.sharded` names the mode, the
exchange and the partition; with `--full` it also reports, per rank, the compute-only time, the bytes per link and the exchange
left exposed in pipelined and in latency mode (PTB_BENCH_SHARDED_MODE=sync makes latency mode the headline).  Rank 0 prints one
JSON line.
"""
import argparse
import gc
import json
import os
import sys
import time

# the host driver only supports dmabuf IPC: without this RCCL / cross-process tensor sharing fails (hipIpcGetMemHandle)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

IMAGE = (5000, 5000, 3)
TILE, STEP, CHANNELS, VIEWS, BATCH = 512, 256, 4, 8, int(os.environ.get("PTB_BENCH_BATCH", "8"))   # (BASELINE: batches of 8; the env override is a diagnostic)
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (guides/MI355X_MICROARCH.md: 8.0 TB/s spec, ~6.3 TB/s achievable)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="after the headline, also run the checks and side measurements: parity with the plain "
                    "merger, API variants, roofline and read ceiling, placement search, secondary configs, CPU baselines (N > 1: band "
                    "parity before timing, exchange cost)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--workload", default="cfg2", choices=["cfg2", "cfg5"], help="cfg2 (default): the headline tiled + d4 merge (BASELINE "
                    "configs[1], sharded over the ranks = configs[2]); cfg5: multiscale 0.75/1.0/1.25 + fliplr TTA, gmean, on 4096x4096 "
                    "(BASELINE configs[4]), output row strips over the ranks")
    ap.add_argument("--chunk-rows", type=int, default=0, help="override the view-kernel chunk rows (16|32|64)")
    ap.add_argument("--memset-accumulators", action="store_true", help="A/B: zero the accumulators with a memset each step instead of first-touch stores")
    ap.add_argument("--placement-tries", type=int, default=8, help="with --full: candidate placements of the model-output pool tried after the "
                    "headline (1 = no search)")
    ap.add_argument("--tunable", action="append", default=[], help="key=value passed to ptb_set_tunable (A/B experiments)")
    ap.add_argument("--unplanned", action="store_true", help="A/B: TileMerger without crops= (lazily built norm_mask + separate merge pass)")
    ap.add_argument("--no-defer", action="store_true", help="A/B: planned merger without deferred band merging (accumulators in HBM)")
    ap.add_argument("--ramp-ms", type=float, default=400.0, help="minimum untimed GPU work before the warm-up; the ramp then goes on (bounded by "
                    "--ramp-max-ms) until three consecutive groups of 10 steps agree within 1.5 %%: a fresh box needs a moment to leave its "
                    "low-power state and to fault the 12 GB of model outputs in")
    ap.add_argument("--ramp-max-ms", type=float, default=4000.0)
    ap.add_argument("--repeats", type=int, default=5, help="the K timed steps are run this many times (each run bracketed by barrier + "
                    "synchronize); `value` is the MEDIAN run, all runs are listed in config.repeat_ms_per_step")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip config.secondary (cfg4 losses, cfg5 multiscale, Lovasz on this GPU)")
    ap.add_argument("--no-variants", action="store_true", help="with --full: skip the secondary timings (no-defer / unplanned / literal drop-in sequence)")
    ap.add_argument("--defer-rows", type=int, default=0, help="rows of the image merged per deferred launch (0: the library default, 1024)")
    ap.add_argument("--diag", action="store_true", help="print per-step / per-call timing diagnostics to stderr")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the timed path returned in its "
                    "last timed step as DIR/<name>.npy (float32 / float64; an output of more than 4 Mi values as the values at a fixed, "
                    "seeded set of positions, DIR/<name>_sample.npy): the inputs are seeded, so two builds run with the same arguments "
                    "can be compared output for output (single GPU only)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.gpus != 1:
        ap.error("--dump-outputs covers the single-GPU path (--gpus 1)")
    return args


DUMP_SAMPLE = 1 << 22          # --dump-outputs: values kept of a larger output (16 MiB in float32)
DUMP_LIMIT = 64 << 20          # bytes written in all
DUMP_SEED = 20240611


def dump_outputs(dirname, outputs):
    """--dump-outputs: every tensor of ``outputs`` ({name: device tensor}) as ``dirname/<name>.npy`` in float32 (float64 stays float64).
    A tensor of more than DUMP_SAMPLE values is written as its values at sorted positions of the flattened tensor drawn from a
    fixed seed (duplicates dropped), ``<name>_sample.npy``: the same positions in every run for the same shape."""
    arrays = {}
    for name, t in outputs.items():
        flat = t.detach().reshape(-1)
        if flat.numel() > DUMP_SAMPLE:
            pos = np.unique(np.random.default_rng(DUMP_SEED).integers(0, flat.numel(), DUMP_SAMPLE))
            flat, name = flat[torch.from_numpy(pos).to(flat.device)], name + "_sample"
        else:
            flat = flat.reshape(t.shape)
        arrays[name] = flat.to(torch.float64 if flat.dtype == torch.float64 else torch.float32).cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT, f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT} byte limit"
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
    print(f"[bench] --dump-outputs: {', '.join(f'{n}.npy {a.shape}' for n, a in arrays.items())} -> {dirname}", file=sys.stderr, flush=True)


def self_launch(args):
    """`python bench.py --gpus N` outside torch.distributed.run: start the N ranks ourselves (one per GPU, this node) and hand
    their exit code on; the ranks' stdout -- rank 0's JSON line last -- passes through."""
    import socket
    import subprocess

    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print("[bench] --gpus", args.gpus, "without WORLD_SIZE: launching", " ".join(cmd), file=sys.stderr, flush=True)
    return subprocess.run(cmd, cwd=ROOT).returncode


def cpu_baseline(slicer, max_seconds=25.0):
    """The reference's own CPU data flow (oracle/torch_chain.py: chunk + inverse views + stack + mean, sequential slice
    `+=`, image / norm_mask -- tta.py:442-467, tiles.py:321-346 -- as multi-threaded torch-CPU ops on all physical cores of this
    host) over the tiles of ONE whole image (same geometry, same batch size); stops early after `max_seconds` and extrapolates
    the remaining batches, so a `--full` run stays bounded on a slow host.  kind = "port": the reference package itself
    does not exist on the GPU box; in the build container the same chain was timed next to the unmodified reference
    (BASELINE.md / DESIGN.md section 5)."""
    from oracle import torch_chain as TC

    cores, logical, model = TC.host_description()
    prev = torch.get_num_threads()
    try:
        g = torch.Generator().manual_seed(0)
        sample = torch.randn((VIEWS * BATCH, CHANNELS, TILE, TILE), generator=g)
        # thread count: these are bandwidth-bound elementwise ops on 33 MB operands, and on a many-core host the thread
        # pool's fork/join costs more than it buys (128 threads on a 2 x 64-core EPYC: 2.6 MP/s, 16 threads: ~3x that), so the
        # baseline uses the fastest of {8, 16, 32, 64, all physical cores} on two probe batches -- the best this host can do
        probe = TC.Merger(slicer.target_shape, CHANNELS, slicer.weight)
        trials = {}
        for nthreads in sorted({min(cores, n) for n in (8, 16, 32, 64, cores)}):
            torch.set_num_threads(nthreads)
            TC.image_deaugment(sample, "d4", "mean")   # (thread pool start-up is not part of the measurement)
            t0 = time.perf_counter()
            for b0 in (0, BATCH):
                probe.integrate_batch(TC.image_deaugment(sample, "d4", "mean"), slicer.crops[b0:b0 + BATCH])
            trials[nthreads] = time.perf_counter() - t0
        del probe
        used = min(trials, key=trials.get)
        torch.set_num_threads(used)
        merger = TC.Merger(slicer.target_shape, CHANNELS, slicer.weight)
        TC.image_deaugment(sample, "d4", "mean")
        n_tiles, done = len(slicer.crops), 0
        t0 = time.perf_counter()
        for b0 in range(0, n_tiles, BATCH):
            crops = slicer.crops[b0:b0 + BATCH]
            nb = len(crops)
            x = sample if nb == BATCH else sample.view(VIEWS, BATCH, CHANNELS, TILE, TILE)[:, :nb].reshape(VIEWS * nb, CHANNELS, TILE, TILE)
            merger.integrate_batch(TC.image_deaugment(x, "d4", "mean"), crops)
            done += nb
            if time.perf_counter() - t0 > max_seconds:
                break
        t_tiles = (time.perf_counter() - t0) * n_tiles / done
        t0 = time.perf_counter()
        merger.merge()
        t_merge = time.perf_counter() - t0
    finally:
        torch.set_num_threads(prev)
    per_image = t_tiles + t_merge
    return {
        "value": round(IMAGE[0] * IMAGE[1] / 1e6 / per_image, 3),
        "unit": "MP/s",
        "cores": used,
        "kind": "port",
        "sample": f"{done} of {n_tiles} tiles in batches of {BATCH} (d4 de-augment: chunk + inverse views + stack + mean; sequential "
                  f"integrate; one full merge) as torch-CPU ops with {used} threads (the fastest of "
                  f"{ {k: round(v, 2) for k, v in trials.items()} } s per two probe batches) on {model} ({cores} physical cores, {logical} "
                  f"logical CPUs), {per_image:.2f} s per image" + ("" if done == n_tiles else " (extrapolated)"),
    }


def _gpu_ms(fn, reps, warm=3, ramp_ms=0.0):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ramp_ms:     # (the GPU idled during the CPU baseline: back to its clocks first)
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def secondary_workloads(dev, with_cpu=True, cpu_budget_s=12.0):
    """The other BASELINE configs on this GPU, driver-visible (bounded: < 3 s of GPU work, ~10 s of CPU baselines):
    configs[3] fused BinaryFocal + Dice + Jaccard on [32,16,512,512] (forward, forward + backward), configs[4] multiscale
    (0.75 / 1.0 / 1.25) + fliplr on 4096 x 4096 with gmean (one-pass kernel and the composed reference call sequence), and the
    Lovasz-softmax loss on [4,16,512,512].  Per entry: ms per call (HIP events around back-to-back calls, module call = every launch
    it makes), the algorithmic bytes of SURVEY 8d (inputs read once + outputs written once), their fraction of the 8 TB/s peak, and
    the reference's op chain timed on the host CPU (oracle/torch_chain.py, a bounded sample, scaled)."""
    from pytorch_toolbelt_amd import losses as L
    from pytorch_toolbelt_amd.inference import tta

    out = {}

    def entry(ms, nbytes, **extra):
        d = {"ms": round(ms, 4), "bytes": int(nbytes), "frac": round(nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        d.update(extra)
        return d

    g = torch.Generator(device=dev).manual_seed(0)
    # ---- configs[3]
    B, C, H, W = 32, 16, 512, 512
    x = torch.randn((B, C, H, W), device=dev, generator=g)
    labels = torch.randint(0, C, (B, H, W), device=dev, generator=g)
    fwd_bytes = x.numel() * 4 + labels.numel() * 8                      # 603 979 776
    bwd_bytes = fwd_bytes + x.numel() * 4                               # + one more read of logits and labels, the gradient written
    crit = L.FocalDiceJaccardLoss("multiclass")
    with torch.no_grad():
        t_f = _gpu_ms(lambda: crit(x, labels), 100, ramp_ms=400.0)
    xg = x.clone().requires_grad_(True)

    def fwd_bwd():
        xg.grad = None
        crit(xg, labels).backward()

    t_fb = _gpu_ms(fwd_bwd, 40)
    out["cfg4_fwd"] = entry(t_f, fwd_bytes, what="FocalDiceJaccardLoss('multiclass') forward, [32,16,512,512] fp32 logits + int64 labels, per module call")
    out["cfg4_fwd_bwd"] = entry(t_fb, fwd_bytes + bwd_bytes, what="same, forward + backward (gradient wrt the logits)")
    seps = {"BinaryFocalLoss": L.BinaryFocalLoss(), "DiceLoss": L.DiceLoss("multiclass"), "JaccardLoss": L.JaccardLoss("multiclass")}
    with torch.no_grad():
        out["cfg4_fwd"]["separate_modules_ms"] = {k: round(_gpu_ms(lambda c=c: c(x, labels), 10), 4) for k, c in seps.items()}
    del xg
    # ---- Lovasz
    probs = torch.softmax(x[:4], 1).contiguous()
    lab4 = labels[:4].contiguous()
    lov = L.LovaszLoss()
    lov_in = probs.numel() * 4 + lab4.numel() * 8
    with torch.no_grad():
        t_lf = _gpu_ms(lambda: lov(probs, lab4), 20)
    pg = probs.clone().requires_grad_(True)

    def lov_fb():
        pg.grad = None
        lov(pg, lab4).backward()

    t_lfb = _gpu_ms(lov_fb, 20)
    # The roofline of a SORT is not its inputs read once: an LSD radix sort of 32-bit keys in 8-bit digits moves every element four
    # times.  Bytes the implemented pipeline has to move (n = 16.8 M elements, 4 B per key / value / gradient):
    #   forward without gradient (key-only sort, ptb_lovasz_fwd_keys; round 6: the last level ranks instead of scattering): error kernel
    #     (pred + labels in, keys out) + 3 histogram reads (pass 0's histogram comes out of the error kernel) + 3 x (keys in + keys out)
    #     + the rank-dot kernel's one read  = lov_in + 11 x 4n   (round 5: 4 scatters + foreground count + dot = lov_in + 14 x 4n)
    #   forward + backward (pair sort + binned gradient): error (pred + labels in, keys out) + 3 histogram reads + first pass (keys in,
    #     pairs out: it makes the values) + 3 x (pairs in + pairs out) + binning pass (count: values in; scatter: values + error keys
    #     in, pairs out -- it also evaluates the loss) + backward (pairs + pred + labels in, gradient out)
    #     = 2 x lov_in + (1 + 3 + 3 + 12 + 1 + 4 + 3) x 4n = 2 x lov_in + 27 x 4n
    n_el = probs.numel()
    lov_sort_fwd = lov_in + 11 * 4 * n_el
    lov_sort_fb = 2 * lov_in + 27 * 4 * n_el
    out["lovasz_fwd"] = entry(t_lf, lov_sort_fwd, what="LovaszLoss() forward on [4,16,512,512] probabilities under no_grad: 16 segments of 1 M elements, key-only "
                                                       "LSD radix sort (three scatters, the last level evaluated from ranks); `bytes` = what the sort pipeline must move (error kernel + 3 "
                                                       "histogram reads + 3 x keys in / out + the rank-dot read), `frac` against 8 TB/s", inputs_once_bytes=int(lov_in))
    out["lovasz_fwd_bwd"] = entry(t_lfb, lov_sort_fb, what="same, forward + backward: (key, index) pair sort + gradient binned by pixel block; `bytes` = error (keys out) + "
                                                           "3 histogram reads + first pass (keys in, pairs out) + 3 x pairs in / out + binning pass (which also "
                                                           "evaluates the loss) + backward",
                                  inputs_once_bytes=int(lov_in + probs.numel() * 4))
    del pg, probs
    # ---- BASELINE.md section 3, second row: integrate + merge only (no TTA) at the headline geometry -- the reference's plain loop
    # `merger.integrate_batch(model(tiles), crops)` ... `merger.merge()` (tiles.py:321-346), a new TileMerger(shape, C, weight) per
    # image, library defaults (from the second image of the geometry the mergers plan themselves: deferred bands, identity view)
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer, TileMerger

    slicer = ImageSlicer(IMAGE, TILE, STEP, weight="pyramid")
    crops = slicer.crops
    preds = [torch.randn((min(BATCH, len(crops) - b0), CHANNELS, TILE, TILE), device=dev, generator=g) for b0 in range(0, len(crops), BATCH)]
    pred_crops = [crops[b0:b0 + BATCH] for b0 in range(0, len(crops), BATCH)]
    plain_bytes = len(crops) * CHANNELS * TILE * TILE * 4 + CHANNELS * slicer.target_shape[0] * slicer.target_shape[1] * 4      # 1 933 574 144

    def plain_image(**kw):
        m = TileMerger(slicer.target_shape, CHANNELS, slicer.weight, device=dev, **kw)
        for t, c in zip(preds, pred_crops):
            m.integrate_batch(t, c)
        plain_image.mode = m.mode
        return m.merge()

    want_plain = plain_image(auto_plan=False)
    t_inc = _gpu_ms(lambda: plain_image(auto_plan=False), 20)
    plain_image()                                                      # the geometry's first image: learnt
    t_self = _gpu_ms(plain_image, 20)
    same = bool(torch.equal(plain_image(), want_plain))
    out["no_tta_5000"] = entry(t_self, plain_bytes, what="integrate_batch(pred, crops) in batches of 8 tiles + merge() on a 5000x5000 image (361 tiles, C = 4, no TTA), "
                                                         "new TileMerger(shape, C, weight) per image on the library's defaults (BASELINE.md section 3: 1 933 574 144 "
                                                         "algorithmic bytes)", merger_mode=plain_image.mode, bit_identical_to_incremental=same,
                               incremental_ms=round(t_inc, 4), incremental_frac=round(plain_bytes / (t_inc * 1e-3) / 1e9 / HBM_PEAK_GBS, 4))
    del preds, want_plain
    # ---- configs[4]
    n, c5 = 4096, 4
    offs = [-n // 4, 0, n // 4]
    ys = [torch.rand((2, c5, n + o, n + o), device=dev, generator=g) * 0.9 + 0.05 for o in offs]
    alg5 = sum(y.numel() for y in ys) * 4 + c5 * n * n * 4               # 1 946 157 056
    for name, red in (("cfg5_gmean", "gmean"), ("cfg5_mean", "mean")):
        t_one = _gpu_ms(lambda: tta.ms_flips_image_deaugment(ys, offs, group="fliplr", inner_reduction=red, reduction=red, align_corners=False), 40,
                        ramp_ms=100.0)
        lit = lambda: tta.ms_image_deaugment([tta.fliplr_image_deaugment(y, reduction=red) for y in ys], offs, reduction=red, align_corners=False)  # noqa: E731
        t_lit = _gpu_ms(lit, 20)
        prev_lazy = tta.set_lazy_deaugment(False)
        try:
            t_eager = _gpu_ms(lit, 10)
        finally:
            tta.set_lazy_deaugment(prev_lazy)
        out[name] = entry(t_one, alg5, what=f"multiscale 0.75/1.0/1.25 + fliplr on 4096x4096, C=4, {red}: tta.ms_flips_image_deaugment (one pass)",
                          literal_composition_ms=round(t_lit, 4), literal_composition_eager_ms=round(t_eager, 4),
                          note="literal_composition = the reference's calls ms_image_deaugment([fliplr_image_deaugment(y_s) ...]): the lazy "
                               "handles are fused into the same one-pass kernel; _eager = lazy handles off (3 de-augment launches + the merge)")
    # ---- SURVEY 8d secondary region, end to end: uint8 image -> (H2D) -> tiles + d4 augment -> model -> de-augment + integrate ->
    # merge + crop -> (D2H), the README loop written literally (a new TileMerger per image, integrate_batch(d4_image_deaugment(y))),
    # with a stand-in model that costs next to nothing (the config's "dummy UNet" would be 90 % of the time and is not this library)
    ys_cpu = [y[:, :1].cpu() for y in ys] if with_cpu else None
    del ys
    torch.cuda.empty_cache()
    try:
        import numpy as np_

        from pytorch_toolbelt_amd.inference.tiles import CudaTileMerger, ImageSlicer

        image = torch.from_numpy(np_.random.default_rng(0).integers(0, 256, IMAGE, dtype=np_.uint8)).pin_memory()
        tiler = ImageSlicer(IMAGE, TILE, STEP, weight="pyramid")
        inv255 = [1.0 / 255.0] * 3

        def stand_in_model(xb):        # [8 views * B, 3, 512, 512] -> [.., 4, 512, 512]: three channels passed through + their mean
            yb = torch.empty((xb.shape[0], CHANNELS, TILE, TILE), device=dev)
            yb[:, :3] = xb
            torch.mean(xb, dim=1, out=yb[:, 3])
            return yb

        def e2e_image():
            dimg = image.to(dev, non_blocking=True)
            merger = CudaTileMerger(tiler.target_shape, CHANNELS, tiler.weight)
            for b0 in range(0, len(tiler.crops), BATCH):
                xb = tiler.split_device(dimg, slice(b0, b0 + BATCH), augment="d4", scale=inv255, bias=[0.0] * 3)
                merger.integrate_batch(tta.d4_image_deaugment(stand_in_model(xb)), tiler.crops[b0:b0 + BATCH])
            return merger.merge_crop(tiler, argmax=True, dtype=torch.uint8).cpu()

        with torch.no_grad():
            for _ in range(3):
                lab_img = e2e_image()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                lab_img = e2e_image()
            t_e2e = (time.perf_counter() - t0) / 3
        assert lab_img.shape == (IMAGE[0], IMAGE[1]) and int(lab_img.max()) < CHANNELS
        out["e2e_5000_stand_in_model"] = {
            "ms": round(t_e2e * 1e3, 2), "MP_s": round(IMAGE[0] * IMAGE[1] / 1e6 / t_e2e, 1),
            "what": "wall clock per 5000x5000x3 uint8 image, host to host: pinned H2D of the image (75 MB), ImageSlicer.split_device (tiles + "
                    "normalise + d4 augment, one launch per 8 tiles), a stand-in model (channel copy + mean: elementwise torch ops), the literal "
                    "integrate_batch(tta.d4_image_deaugment(y), crops) on a new TileMerger per image, merge_crop(argmax, uint8) and its D2H (25 MB)"}
        del image, lab_img
    except Exception as exc:  # noqa: BLE001
        out["e2e_5000_stand_in_model"] = {"error": repr(exc)}
    if os.environ.get("PTB_BENCH_UNET", "1") == "1":
        try:
            out["e2e_5000_unet"] = e2e_unet(dev)
        except Exception as exc:  # noqa: BLE001
            out["e2e_5000_unet"] = {"error": repr(exc)}
    if with_cpu:
        from oracle import torch_chain as TC

        cores, _logical, model = TC.host_description()
        prev = torch.get_num_threads()
        try:
            torch.set_num_threads(min(cores, 32))
            used = torch.get_num_threads()
            xs, ls = x[:2].cpu(), labels[:2].cpu()
            TC.binary_focal_multiclass_dice_jaccard(xs[:1], ls[:1])
            t0 = time.perf_counter()
            TC.binary_focal_multiclass_dice_jaccard(xs, ls)
            t_c4 = (time.perf_counter() - t0) * (B / 2)
            out["cfg4_fwd"]["cpu_baseline"] = {"ms": round(t_c4 * 1e3, 1), "cores": used, "kind": "port",
                                               "sample": f"2 of {B} images through the reference's op chain (one-hot focal + Dice + Jaccard), x{B // 2}; {model}"}
            p1, l1 = torch.softmax(xs[:1], 1), ls[:1]
            t0 = time.perf_counter()
            TC.lovasz_softmax(p1, l1)
            t_lv = (time.perf_counter() - t0) * 4
            out["lovasz_fwd"]["cpu_baseline"] = {"ms": round(t_lv * 1e3, 1), "cores": used, "kind": "port",
                                                 "sample": "1 of 4 images (16 classes: sort + cumsum + dot per class), x4"}
            if time.perf_counter() - t0 < cpu_budget_s:
                t0 = time.perf_counter()
                TC.ms_fliplr_deaugment(ys_cpu, offs, "gmean", align_corners=False)
                t_c5 = (time.perf_counter() - t0) * c5
                out["cfg5_gmean"]["cpu_baseline"] = {"ms": round(t_c5 * 1e3, 1), "cores": used, "kind": "port",
                                                     "sample": f"1 of {c5} channels (flip + stack + gmean per scale, F.interpolate, stack + gmean), x{c5}"}
        finally:
            torch.set_num_threads(prev)
    return out


def _unet(width=32, classes=CHANNELS):
    """BASELINE configs[1]'s "dummy 4-class UNet" as plain torch: the reference's UnetBlock (two conv3x3 without bias, each
    followed by BatchNorm + ReLU: modules/unet.py:10-47) in a 4-level encoder (32 / 64 / 128 / 256 features, 2 x 2 max-pool between the
    levels: modules/encoders/unet.py:13-52) and decoder (nearest 2 x up-sampling, concatenation with the skip, UnetBlock:
    modules/decoders/unet.py:24-129), 1 x 1 head; 3 -> 4 channels, manual_seed(0), eval()."""
    from torch import nn

    def block(cin, cout):
        return nn.Sequential(nn.Conv2d(cin, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True),
                             nn.Conv2d(cout, cout, 3, padding=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(inplace=True))

    class UNet(nn.Module):
        def __init__(self):
            super().__init__()
            w = [width, width * 2, width * 4, width * 8]
            self.enc = nn.ModuleList([block(3, w[0]), block(w[0], w[1]), block(w[1], w[2]), block(w[2], w[3])])
            self.dec = nn.ModuleList([block(w[3] + w[2], w[2]), block(w[2] + w[1], w[1]), block(w[1] + w[0], w[0])])
            self.head = nn.Conv2d(w[0], classes, 1)

        def forward(self, x):
            feats = []
            for i, e in enumerate(self.enc):
                x = e(x if i == 0 else nn.functional.max_pool2d(x, 2))
                feats.append(x)
            for d, skip in zip(self.dec, feats[-2::-1]):
                x = d(torch.cat([nn.functional.interpolate(x, scale_factor=2, mode="nearest"), skip], 1))
            return self.head(x)

    torch.manual_seed(0)
    return UNet().eval()


def e2e_unet(dev):
    """SURVEY 8d's secondary region with the model BASELINE names: uint8 5000 x 5000 x 3 image host -> (H2D) -> tiles + normalise + d4
    augment (split_device) -> 4-level UNet (random weights, eval) -> d4 de-augment + integrate -> merge + crop + arg-max -> (D2H), batches
    of 8 tiles x 8 views, ONE timed image per variant after a warm-up on the first two batches and the ragged last one (MIOpen picks its
    convolution algorithms per shape there; ~20 s per dtype on a fresh box, untimed).  Variants: the reference's literal calls on a new TileMerger per image (fp32); the planned +
    deferred merger (crops= known, defer=True; fp32); the same with the model under bf16 autocast, its bfloat16 outputs read natively
    by the band kernel; the literal calls under bf16 autocast (lazy handle of a bfloat16 tensor, fused with PTB_ROUND_SRC).  The model is ~99.9 % of the time: MP/s says what a user gets end to end, `merge_share` what the library
    costs inside it, `peak_GB` what holding batches (defer) adds next to the UNet's activations."""
    import numpy as np_

    from pytorch_toolbelt_amd.inference import tta
    from pytorch_toolbelt_amd.inference.tiles import CudaTileMerger, ImageSlicer

    image = torch.from_numpy(np_.random.default_rng(0).integers(0, 256, IMAGE, dtype=np_.uint8)).pin_memory()
    tiler = ImageSlicer(IMAGE, TILE, STEP, weight="pyramid")
    model = _unet().to(dev)
    inv255 = [1.0 / 255.0] * 3
    n = len(tiler.crops)

    def run(kind, autocast_dtype, batches=None):
        dimg = image.to(dev, non_blocking=True)
        if kind == "literal" or batches is not None:      # (the warm-up skips batches: not a sequence a planned merger may see)
            merger = CudaTileMerger(tiler.target_shape, CHANNELS, tiler.weight)
        else:
            merger = CudaTileMerger(tiler.target_shape, CHANNELS, tiler.weight, crops=tiler.crops, defer=True)
        ctx = torch.autocast("cuda", dtype=autocast_dtype) if autocast_dtype is not None else torch.autocast("cuda", enabled=False)
        starts = list(range(0, n, BATCH))
        for b0 in (starts if batches is None else starts[:batches] + starts[-1:]):      # (warm-up: the first batches + the ragged last one)
            xb = tiler.split_device(dimg, slice(b0, b0 + BATCH), augment="d4", scale=inv255, bias=[0.0] * 3)
            with ctx:
                yb = model(xb)
            if kind == "literal":
                merger.integrate_batch(tta.d4_image_deaugment(yb), tiler.crops[b0:b0 + BATCH])
            else:
                merger.integrate_batch_deaugment(yb, tiler.crops[b0:b0 + BATCH], group="d4", reduction="mean")
        if batches is not None:
            return None
        return merger.merge_crop(tiler, argmax=True, dtype=torch.uint8).cpu()

    res = {"what": "wall clock per 5000x5000x3 uint8 image, host to host, through the plain-torch 4-level conv3x3-BN-ReLU UNet (3 -> 4 channels, "
                   "32/64/128/256 features, manual_seed(0), eval): 46 batches of 8 tiles x 8 d4 views; one timed image per variant"}
    with torch.no_grad():
        for name, kind, dt in (("literal_fp32", "literal", None), ("deferred_fp32", "deferred", None), ("deferred_bf16_autocast", "deferred", torch.bfloat16),
                               ("literal_bf16_autocast", "literal", torch.bfloat16)):
            run(kind, dt, batches=2)                      # warm-up: MIOpen's algorithm search, allocator
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            labels = run(kind, dt)
            wall = time.perf_counter() - t0
            assert labels.shape == (IMAGE[0], IMAGE[1]) and int(labels.max()) < CHANNELS
            res[name] = {"ms": round(wall * 1e3, 1), "MP_s": round(IMAGE[0] * IMAGE[1] / 1e6 / wall, 2),
                         "peak_GB": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2)}
        # the model alone on the same 46 batches (no merger): what is left of the wall clock is slicing, merging and the copies
        xb = tiler.split_device(image.to(dev), slice(0, BATCH), augment="d4", scale=inv255, bias=[0.0] * 3)
        for name, dt in (("model_only_fp32_ms", None), ("model_only_bf16_autocast_ms", torch.bfloat16)):
            ctx = torch.autocast("cuda", dtype=dt) if dt is not None else torch.autocast("cuda", enabled=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with ctx:
                for _ in range((n + BATCH - 1) // BATCH):
                    model(xb)
            torch.cuda.synchronize()
            res[name] = round((time.perf_counter() - t0) * 1e3, 1)
    return res


def main_cfg5(args):
    """BASELINE configs[4]: multiscale (0.75 / 1.0 / 1.25) + fliplr TTA on 4096 x 4096, gmean inside every scale and across the
    scales, C = 4.  One step = one image: every rank merges its strip of output rows from the rows (with the bilinear taps' halo)
    of the three model outputs it holds -- no collective, the strips of the result stay sharded (parallel.ms_strip_plan, SURVEY 8e:
    the reference's MultiscaleTTA, inference/tta.py:759-801, on one device).  N = 1: the one-pass kernel (ptb_ms_flip_deaug_reduce)."""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = 0 if os.environ.get("PTB_BENCH_SAME_GPU", "0") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    use_dist = world > 1
    if use_dist:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        backend = os.environ.get("PTB_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    import __graft_entry__ as entry

    if rank == 0:
        entry.build()
    if use_dist:
        dist.barrier()
    from pytorch_toolbelt_amd.inference import tta
    from pytorch_toolbelt_amd.parallel import ms_flips_image_deaugment_strip, ms_strip_plan

    n, C, V = 4096, 4, 2
    offs = [-n // 4, 0, n // 4]
    heights = [n + o for o in offs]
    g = torch.Generator(device=dev).manual_seed(1234)
    plan = ms_strip_plan(heights, n, world, align_corners=False)[rank]
    r0, r1 = plan["out"]
    if world == 1:
        ys = [torch.rand((V, C, h, h), device=dev, generator=g) * 0.9 + 0.05 for h in heights]

        def step():
            return tta.ms_flips_image_deaugment(ys, offs, group="fliplr", inner_reduction="gmean", reduction="gmean", align_corners=False)
    else:
        # this rank's rows of every scale's (fliplr-augmented) model output: the strip the model would have produced here
        ys = [torch.rand((V, C, s1 - s0, h), device=dev, generator=g) * 0.9 + 0.05 for (s0, s1), h in zip(plan["src"], heights)]

        def step():      # the same one-pass kernel on this rank's rows (every view of every scale's strip read once)
            return ms_flips_image_deaugment_strip(ys, heights, plan["src"], plan["out"], (n, n), group="fliplr", inner_reduction="gmean",
                                                  reduction="gmean", align_corners=False)

    def sync():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    gc.collect()
    gc.freeze()
    for _ in range(max(args.warmup, 20)):
        step()
    runs = []
    n_runs = max(1, args.repeats)
    for i in range(n_runs):
        sync()
        t0 = time.perf_counter()
        for _ in range(args.steps - 1):
            step()
        out = step()
        sync()
        wall = time.perf_counter() - t0
        if use_dist:
            tmax = torch.tensor([wall], device=dev, dtype=torch.float64)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            wall = float(tmax.item())
        runs.append(wall)
        if args.dump_outputs and i == n_runs - 1:     # what the last timed step returned
            dump_outputs(args.dump_outputs, {"merged": out})
        del out
    elapsed = sorted(runs)[len(runs) // 2]
    ms_per_step = elapsed / args.steps * 1e3
    my_bytes = sum(y.numel() for y in ys) * 4 + C * (r1 - r0) * n * 4
    line = None
    if rank == 0:
        line = {
            "metric": "megapixels/sec multiscale(0.75/1.0/1.25)+fliplr TTA gmean merge on 4096x4096", "value": round(n * n / 1e6 * args.steps / elapsed, 1),
            "unit": "MP/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "BASELINE cfg5: 4096x4096, scales 0.75/1.0/1.25 (offsets -1024, 0, +1024), fliplr TTA inside every scale (2 views), "
                                   "gmean / gmean, C=4 model outputs resident in HBM; " +
                                   ("one pass (tta.ms_flips_image_deaugment)" if world == 1 else
                                    f"output rows split over {world} ranks (parallel.ms_strip_plan: np.linspace rows, each rank holds the source rows "
                                    "its taps touch), per rank ONE launch of the one-pass kernel on its strips (ms_flips_image_deaugment_strip); no collective"),
                       "parallelism": "single GPU" if world == 1 else f"row strips over {world} ranks", "rank0_out_rows": [r0, r1],
                       "repeat_ms_per_step": [round(w / args.steps * 1e3, 4) for w in runs]},
            "roofline": {"kernel": "ms_flip_reduce_kernel (one pass)" if world == 1 else "ms_flip_reduce_kernel on rank 0's row strip (one pass)",
                         "bound": "hbm", "achieved": round(my_bytes / (ms_per_step * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(my_bytes / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "traffic": None,
                         "algorithmic_bytes_per_launch": my_bytes, "avg_launch_ms": round(ms_per_step, 5)},
        }
        if args.full and world == 1 and not args.no_cpu_baseline:
            from oracle import torch_chain as TC

            cores, _logical, model = TC.host_description()
            prev = torch.get_num_threads()
            torch.set_num_threads(min(cores, 32))
            ys_cpu = [y[:, :1].cpu() for y in ys]
            t0 = time.perf_counter()
            TC.ms_fliplr_deaugment(ys_cpu, offs, "gmean", align_corners=False)
            per_image = (time.perf_counter() - t0) * C
            torch.set_num_threads(prev)
            line["cpu_baseline"] = {"value": round(n * n / 1e6 / per_image, 3), "unit": "MP/s", "cores": min(cores, 32), "kind": "port",
                                    "sample": f"1 of {C} channels through the reference's op chain (x{C}); {model}"}
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        import ctypes

        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(json.dumps(line), flush=True)


def main():
    args = parse()
    if args.workload == "cfg5":
        return main_cfg5(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        sys.exit(self_launch(args))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    if os.environ.get("PTB_BENCH_SAME_GPU", "0") == "1":   # functional test of the N > 1 path on a 1-GPU box (with gloo)
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    force_sharded = os.environ.get("PTB_BENCH_FORCE_SHARDED", "0") == "1"  # exercise the RCCL path with any world size
    use_dist = world > 1 or force_sharded
    if use_dist:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        backend = os.environ.get("PTB_BENCH_BACKEND", "nccl")   # "nccl" is RCCL on ROCm
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"

    import __graft_entry__ as entry

    if rank == 0:
        entry.build()
    if use_dist:
        dist.barrier()
    from pytorch_toolbelt_amd import _native as N
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer, TileMerger
    from pytorch_toolbelt_amd.parallel import ShardedTileMerger

    if args.chunk_rows:
        assert N.load().ptb_set_tunable(0, args.chunk_rows) == 0
    for kv in args.tunable:
        k, v = kv.split("=")
        assert N.load().ptb_set_tunable(int(k), int(v)) == 0

    slicer = ImageSlicer(IMAGE, TILE, STEP, weight="pyramid")
    n_tiles = len(slicer.crops)
    assert n_tiles == 361 and slicer.target_shape == (5120, 5120)

    # ---- this rank's share of the tiles, and their (synthetic) model outputs resident in HBM -------------------
    sharded = use_dist
    if args.dump_outputs and sharded:
        sys.exit("bench.py: --dump-outputs covers the single-device merge, not the sharded one")
    planned = deferred = False
    fallback = None   # set when the requested merger could not be used and a slower one was (reported in the JSON line)
    partition = os.environ.get("PTB_BENCH_PARTITION", "tiles")   # "tiles": 45 / 46 tiles per rank at N = 8; "rows": whole tile rows
    if not sharded:
        my_tiles = np.arange(n_tiles)
    else:
        # default: under nccl the rectangles travel as ONE ncclGroup posted from C on the library's own communicator (falls back to
        # torch.distributed p2p on every rank alike when RCCL cannot be bound); PTB_BENCH_EXCHANGE=torch forces batch_isend_irecv
        exchange = {"auto": "auto", "rccl": "auto", "torch": None}[os.environ.get("PTB_BENCH_EXCHANGE", "auto")]
        sharded_merger = ShardedTileMerger(slicer.target_shape, CHANNELS, slicer.weight, slicer.crops, device=dev, partition=partition,
                                           defer=os.environ.get("PTB_BENCH_SHARDED_DEFER", "1") == "1", exchange=exchange)
        my_tiles = sharded_merger.tiles
    crops = slicer.crops[my_tiles]
    batches = [(b0, min(len(crops), b0 + BATCH)) for b0 in range(0, len(crops), BATCH)]
    def alloc_outputs(pad_mb):
        """The (synthetic) model outputs of this rank's tiles, resident in HBM: (batch tensors, allocations to keep alive)."""
        keep = [torch.empty(pad_mb << 20, device=dev, dtype=torch.uint8)] if pad_mb else []
        if os.environ.get("PTB_BENCH_ONE_BUFFER", "0") == "1":   # A/B: all model outputs as slices of one 12.1 GB allocation
            outputs = torch.empty((VIEWS * len(crops), CHANNELS, TILE, TILE), device=dev, dtype=torch.float32)
            tensors = [outputs[VIEWS * b0:VIEWS * b1] for b0, b1 in batches]
        else:   # like a model would leave them: one tensor per batch (chunk-major: view k of tile j at row k * nb + j)
            if os.environ.get("PTB_BENCH_PRIME_POOL", "1") == "1":
                # One reservation for the whole image's outputs, handed back to torch's caching allocator right away: the per-batch
                # tensors below are then carved out of that ONE device allocation (the allocator splits cached blocks) instead of 46
                # separate 256 MiB hipMallocs (a serving process reserves its memory up front, too).  PTB_BENCH_PRIME_POOL=0: without.
                total = sum(VIEWS * (b1 - b0) for b0, b1 in batches) * CHANNELS * TILE * TILE
                torch.empty(total, device=dev, dtype=torch.float32)
            order = list(range(len(batches)))
            if os.environ.get("PTB_BENCH_SHUFFLE_ALLOC", "0") == "1":   # diagnostics: allocation order != integration order
                np.random.default_rng(7).shuffle(order)
            tensors = [None] * len(batches)
            for i in order:
                b0, b1 = batches[i]
                tensors[i] = torch.empty((VIEWS * (b1 - b0), CHANNELS, TILE, TILE), device=dev, dtype=torch.float32)
        for t, (b0, b1) in zip(tensors, batches):
            fill_outputs(t, my_tiles[b0:b1])
        return tensors, keep

    def fill_outputs(t, tiles):
        """Model outputs of the given tiles (global indices) into the chunk-major batch tensor ``t``: every tile's 8 views x C x 512 x 512
        values come from a generator seeded with the TILE's index, so any rank can reproduce any tile (the parity check below feeds
        a single-device merger the tiles its neighbours own)."""
        nb = len(tiles)
        by_view = t.view(VIEWS, nb, CHANNELS, TILE, TILE)
        tmp = torch.empty((VIEWS, CHANNELS, TILE, TILE), device=dev, dtype=torch.float32)
        g = torch.Generator(device=dev)
        for j, tile in enumerate(tiles):
            g.manual_seed(1234 + int(tile))
            tmp.normal_(generator=g)
            by_view[:, j] = tmp

    batch_tensors, _keep = alloc_outputs(int(os.environ.get("PTB_BENCH_PAD_MB", "0")))   # (the pad: a placement diagnostic)
    batch_crops = [crops[b0:b1] for b0, b1 in batches]

    if not sharded:
        # planned merger: the slicer's crop list is known before the first batch (the README loop has it), so every
        # block is divided by the precomputed normaliser in the launch that brings its last tile and merge() returns the
        # finished map (+3 % per image; --unplanned: lazily built normaliser + separate merge pass)
        planned = not (args.unplanned or args.memset_accumulators)
        # deferred bands (default): the merger keeps references to the batches (they stay resident and unmodified here) and
        # merges each group of bands (1024 rows) of the image in ONE launch when its last tile has arrived -- no accumulator in HBM
        deferred = planned and not args.no_defer
        merger = TileMerger(slicer.target_shape, CHANNELS, slicer.weight, device=dev, crops=slicer.crops if planned else None, defer=deferred,
                            defer_rows=args.defer_rows or None)
    else:
        merger = sharded_merger

    def step():
        if not sharded:
            if args.memset_accumulators:
                merger.image.zero_()      # (property access materialises -> every later write is a read-modify-write)
                merger.norm_mask.zero_()
            else:
                merger.reset()  # first-touch accumulators: logically zero, no memset
            for t, c in zip(batch_tensors, batch_crops):
                merger.integrate_batch_deaugment(t, c, group="d4", reduction="mean")
            return merger.merge()
        if pipelined:
            if in_flight[0] is None and merger._result is not None:
                merger.reset()      # (after a synchronous merge() the image still sits in the current buffers)
            # one image per step, pipelined: this image's halo exchange stays in flight while the NEXT step's kernels run (second set
            # of buffers); the previous image is completed here, after this one's tiles were issued.  `drain()` completes the last.
            for t, c in zip(batch_tensors, batch_crops):
                merger.integrate_batch_deaugment(t, c, group="d4", reduction="mean")
            ticket = merger.merge_async()
            prev, in_flight[0] = in_flight[0], ticket
            return prev.result() if prev is not None else None
        merger.reset()
        for t, c in zip(batch_tensors, batch_crops):
            merger.integrate_batch_deaugment(t, c, group="d4", reduction="mean")
        return merger.merge()  # this rank's band of the merged image

    in_flight = [None]
    pipelined = sharded and os.environ.get("PTB_BENCH_SHARDED_MODE", "pipelined") == "pipelined"

    def drain():
        """Complete the image still in flight (pipelined sharded steps): part of every timed region, before its closing synchronize."""
        if in_flight[0] is not None:
            band = in_flight[0].result()
            in_flight[0] = None
            return band
        return None

    def sync():
        drain()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- N > 1, --full: parity before anything is timed.  This rank's band of ONE synchronously merged image against the rows the plain
    # single-device merger produces for the same model outputs (every tile that touches the owned rows, regenerated from its seed,
    # integrated in the single-device order).  "pixel_rows" is bit-identical by construction; tile partitions add the neighbours'
    # partial sums in another association: a few 1e-7 on O(1) values, against the 1e-5 of BASELINE.json.
    parity = None
    if sharded and args.full:
        merger.reset()
        for t, c in zip(batch_tensors, batch_crops):
            merger.integrate_batch_deaugment(t, c, group="d4", reduction="mean")
        band = merger.merge()
        merger.reset()
        diff, checked = 0.0, 0
        owned = merger.owned_rows
        if band is not None and owned is not None and owned[1] > owned[0]:
            o0, o1 = owned
            ys = slicer.crops[:, 1]
            touching = np.nonzero((ys < o1) & (ys + TILE > o0))[0]
            single = TileMerger(slicer.target_shape, CHANNELS, slicer.weight, device=dev, auto_plan=False)
            for b0 in range(0, len(touching), BATCH):
                sel = touching[b0:b0 + BATCH]
                y = torch.empty((VIEWS * len(sel), CHANNELS, TILE, TILE), device=dev, dtype=torch.float32)
                fill_outputs(y, sel)
                single.integrate_batch_deaugment(y, slicer.crops[sel], group="d4", reduction="mean")
            want = single.merge()[:, o0:o1]
            assert bool(torch.isfinite(want).all()), "the single-device merge of the tiles over this rank's rows has uncovered pixels"
            diff = float((band.reshape(want.shape) - want).abs().nan_to_num(nan=float("inf")).max())
            checked = int(want.numel())
            del single, want, y
        torch.cuda.synchronize()
        stats = torch.tensor([diff, float(checked), 1.0 if getattr(merger, "exchange", None) is not None else 0.0], device=dev, dtype=torch.float64)
        worst = stats.clone()
        dist.all_reduce(worst, op=dist.ReduceOp.MAX)
        total = stats.clone()
        dist.all_reduce(total, op=dist.ReduceOp.SUM)
        torch.cuda.empty_cache()
        from pytorch_toolbelt_amd import parallel as _par

        parity = {"parity_max_abs_diff": float(worst[0].item()), "parity_tolerance": 1e-5, "parity_values_checked": int(total[1].item()),
                  "parity_against": "TileMerger (single device, incremental) over every tile touching the rank's rows, same seeded model outputs",
                  "rccl_ranks": int(total[2].item()), "rccl_error": _par.last_exchange_error()}
        if rank == 0:
            print(f"[bench] sharded parity: max|band - single-device| = {parity['parity_max_abs_diff']:.3g} over {parity['parity_values_checked']} values; "
                  f"{parity['rccl_ranks']}/{world} ranks on the library's RCCL exchange", file=sys.stderr, flush=True)

    # Host hygiene: a generation-2 Python GC pass over the ~10^5 objects torch leaves behind takes 30-45 ms (ten
    # steps' worth) and used to land inside the timed region; collect once and freeze the survivors, as a serving loop
    # would after start-up.
    gc.collect()
    gc.freeze()
    if args.diag and rank == 0 and not use_dist:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(41)]
        sync()
        tt = time.perf_counter()
        ev[0].record()
        hs = []
        for i in range(40):
            step()
            ev[i + 1].record()
            hs.append(round((time.perf_counter() - tt) * 1e3, 2))
        sync()
        print(f"[diag] cold start: gpu ms per step {[round(ev[i].elapsed_time(ev[i + 1]), 2) for i in range(40)]}", file=sys.stderr)
        print(f"[diag] cold start: host issue done at ms {hs}", file=sys.stderr)
    if not sharded and planned:
        # one untimed step that is also checked: should the planned path ever misbehave on this box, the benchmark falls
        # back to the ordinary merger (and says so in the JSON) instead of dying
        def probe_ok():
            try:
                probe = step()
                if not bool(torch.isfinite(probe).all()) or merger._plan is None:
                    return False
                if deferred:
                    return merger._bands is not None and merger._defer_active and merger._bands_done == len(merger._bands.bands)
                return bool(merger._plan.done.all())
            except Exception as exc:  # noqa: BLE001
                print(f"[bench] {'deferred' if deferred else 'planned'} merger failed ({exc!r})", file=sys.stderr)
                return False

        if deferred and not probe_ok():
            print("[bench] falling back to the planned merger without deferred bands", file=sys.stderr)
            deferred, fallback = False, "deferred band merger failed its probe step: planned merger without defer used instead"
            merger = TileMerger(slicer.target_shape, CHANNELS, slicer.weight, device=dev, crops=slicer.crops)
        if not deferred and not probe_ok():
            print("[bench] falling back to the unplanned merger", file=sys.stderr)
            planned, fallback = False, "planned merger failed its probe step: unplanned merger used instead"
            merger = TileMerger(slicer.target_shape, CHANNELS, slicer.weight, device=dev)
    # power management: keep a GPU that has been idle (a fresh box, the seconds this process spent importing torch) busy for a
    # moment before the warm-up (untimed, like the build)
    ramp_groups = []
    if use_dist:
        # every rank must run the SAME number of steps (each one exchanges halos): a fixed count, not a wall-clock loop
        for _ in range(60 if args.ramp_ms > 0 else 0):
            step()
        torch.cuda.synchronize()
    else:
        # until the step time has settled: a fresh lease starts in a low-power state and with cold page tables for the 12 GB of
        # model outputs; groups of 10 steps are timed until three in a row agree within 1.5 % (or --ramp-max-ms is spent)
        t_ramp = time.perf_counter()
        while True:
            tg = time.perf_counter()
            for _ in range(10):
                step()
            torch.cuda.synchronize()
            ramp_groups.append((time.perf_counter() - tg) * 100.0)   # ms per step
            spent = (time.perf_counter() - t_ramp) * 1e3
            last = ramp_groups[-3:]
            settled = len(last) == 3 and max(last) <= 1.015 * min(last)
            if (spent >= args.ramp_ms and settled) or spent >= args.ramp_max_ms:
                break
    for _ in range(args.warmup):
        step()
    sync()
    th0 = time.perf_counter()   # host-side cost of issuing one step (no device sync): must stay well below ms_per_step
    step()
    host_ms = (time.perf_counter() - th0) * 1e3
    sync()

    def timed_run(fn, k, keep=None):
        """EXACTLY k steps bracketed by barrier + synchronize on both sides; (wall seconds [max over ranks], HIP-event ms).
        ``keep``: a list that receives what the last step returned (--dump-outputs)."""
        sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(k - 1):
            fn()
        out = fn()
        e1.record()
        sync()
        wall = time.perf_counter() - t0
        if use_dist:
            tmax = torch.tensor([wall], device=dev, dtype=torch.float64)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            wall = float(tmax.item())
        if keep is not None:
            keep.append(out)
        return wall, e0.elapsed_time(e1)

    n_runs = max(1, args.repeats)
    last_out = []     # --dump-outputs: what the last timed step of the last run returned (earlier runs keep nothing alive)
    runs = [timed_run(step, args.steps, keep=last_out if args.dump_outputs and i == n_runs - 1 else None) for i in range(n_runs)]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"merged": last_out.pop()})
    # ---- the headline is measured; what follows up to the JSON line runs with --full only, apart from config.sharded's description.
    # ---- N = 1: the timed path's OUTPUT, checked right after the timed runs against the plain HIP merger (accumulate now, divide in
    # merge(): the reference's data flow, tiles.py:321-346, pinned to the oracle and to the reference's goldens by the -m gpu suite) on
    # the same model outputs: every value of the merged map, not a digest.  Planned and deferred mergers are bit-identical to it.
    parity1 = None
    if args.full and not sharded:
        timed_out = step()
        plain = TileMerger(slicer.target_shape, CHANNELS, slicer.weight, device=dev, auto_plan=False)
        for t, c in zip(batch_tensors, batch_crops):
            plain.integrate_batch_deaugment(t, c, group="d4", reduction="mean")
        want1 = plain.merge()
        parity1 = {"max_abs_diff_vs_plain_merger": float((timed_out - want1).abs().nan_to_num(nan=float("inf")).max()),
                   "bit_identical": bool(torch.equal(timed_out, want1)), "values_checked": int(want1.numel()), "tolerance": 1e-5,
                   "against": "TileMerger(auto_plan=False): one accumulate launch per batch + merge() on the same resident model outputs "
                              "(itself checked against the numpy oracle and the reference's golden vectors by tests/test_fullsize_gpu.py)"}
        del plain, want1, timed_out
        torch.cuda.empty_cache()
    order = sorted(range(len(runs)), key=lambda i: runs[i][0])
    elapsed, region_event_ms = runs[order[len(order) // 2]]    # the median run is the reported one
    repeat_ms = [round(r[0] / args.steps * 1e3, 4) for r in runs]

    # ---- N > 1: how the exchange ran; with --full also what it costs, measured (the same fields tools/shard_sim.py predicts from a
    # one-GPU box)
    sharded_report = None
    if sharded and world > 1:
        from pytorch_toolbelt_amd import parallel as _par

        rccl_error = parity["rccl_error"] if parity is not None else _par.last_exchange_error()
        sharded_report = {
            **(parity or {}),
            "mode": "pipelined (merge_async: image i's exchange under image i+1's kernels)" if pipelined else "latency (merge() joins the exchange inside the image)",
            "exchange": ("ptb_halo_exchange: one ncclGroup per image on the library's own RCCL communicator" if merger.exchange is not None else
                         "torch.distributed.batch_isend_irecv" + ("" if backend == "nccl" and os.environ.get("PTB_BENCH_EXCHANGE", "auto") == "torch" else
                                                                 " (the library's RCCL communicator was NOT used: " + (rccl_error or f"backend {backend}") + ")")),
            "partition": partition,
        }
    if sharded and world > 1 and args.full:
        def sync_step():
            merger.reset()
            for t, c in zip(batch_tensors, batch_crops):
                merger.integrate_batch_deaugment(t, c, group="d4", reduction="mean")
            return merger.merge()

        def mode_ms(fn):
            for _ in range(3):
                fn()
            return sorted(timed_run(fn, args.steps)[0] for _ in range(3))[1] / args.steps * 1e3

        def pipe_step():
            if in_flight[0] is None and merger._result is not None:
                merger.reset()
            for t, c in zip(batch_tensors, batch_crops):
                merger.integrate_batch_deaugment(t, c, group="d4", reduction="mean")
            ticket = merger.merge_async()
            prev, in_flight[0] = in_flight[0], ticket
            return prev.result() if prev is not None else None

        other_ms = mode_ms(sync_step if pipelined else pipe_step)     # the mode that is not the headline
        # compute only: the same steps with the exchange stubbed out on every rank (rectangles packed, nothing sent, the receive
        # buffers used as they are -- wrong pixels on the shared rows, same kernels and bytes)
        real_start = merger._start_exchange

        def stub_exchange():
            merger._exchanged = True

        merger._start_exchange = stub_exchange
        try:
            for _ in range(3):
                sync_step()
            torch.cuda.synchronize()
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record()
            for _ in range(args.steps):
                sync_step()
            c1.record()
            torch.cuda.synchronize()
            compute_ms = c0.elapsed_time(c1) / args.steps
        finally:
            del merger._start_exchange
            assert merger._start_exchange.__func__ is real_start.__func__
        sync()
        mine = {"rank": rank, "tiles": int(len(crops)), "owned_rows": list(merger.owned_rows or (0, 0)), "compute_only_ms": round(compute_ms, 4),
                "out_MB_per_link": {str(d): round((r1 - r0) * (c1_ - c0_) * CHANNELS * 4 / 1e6, 2) for d, r0, r1, c0_, c1_ in merger.sends},
                "in_MB_per_link": {str(s_): round((r1 - r0) * (c1_ - c0_) * CHANNELS * 4 / 1e6, 2) for s_, r0, r1, c0_, c1_ in merger.recvs}}
        everyone = [None] * world
        dist.all_gather_object(everyone, mine)
        ms_now = elapsed / args.steps * 1e3
        slowest_compute = max(e["compute_only_ms"] for e in everyone)
        sharded_report.update({
            "pipelined_ms_per_image": round(ms_now if pipelined else other_ms, 4),
            "latency_mode_ms_per_image": round(other_ms if pipelined else ms_now, 4),
            "slowest_rank_compute_only_ms": round(slowest_compute, 4),
            "exposed_exchange_ms": {"pipelined": round(max((ms_now if pipelined else other_ms) - slowest_compute, 0.0), 4),
                                    "latency_mode": round(max((other_ms if pipelined else ms_now) - slowest_compute, 0.0), 4)},
            "per_rank": everyone,
            "note": "ms per 5000x5000 image over all ranks (max over ranks, barrier + synchronize around K images); compute_only = the same "
                    "steps with the exchange stubbed out; bytes per link = the partial-sum rectangles one rank sends to / receives from one "
                    "neighbour (each pair of GPUs has its own xGMI link, both directions at once); tools/shard_sim.py predicts the same "
                    "fields from one GPU + a link model (profiles/r04_shard_sim.txt)",
        })

    if sharded_report is None and parity is not None:      # (PTB_BENCH_FORCE_SHARDED with one rank)
        sharded_report = parity

    # ---- secondary timings (single GPU): what each API extension of the headline configuration buys, driver-visible
    variants = None
    region_bytes_all = VIEWS * n_tiles * CHANNELS * TILE * TILE * 4 + CHANNELS * 5120 * 5120 * 4   # 12 532 580 352 B
    if args.full and not sharded and not args.no_variants:
        from pytorch_toolbelt_amd.inference import tta as _tta

        from pytorch_toolbelt_amd.inference import tiles as _tiles

        def variant(make, literal=False, fresh=False, eager=False, self_plan=True, tensors=None):
            tensors = batch_tensors if tensors is None else tensors
            prev = (_tta.set_lazy_deaugment(not eager), _tiles.set_auto_plan(self_plan))
            _tiles._auto.clear()
            m = make()            # (after the switches: a merger reads the self-planning setting when it is constructed)

            def vstep():
                nonlocal m
                if fresh:
                    m = make()    # the README loop: a new merger for every image
                else:
                    m.reset()
                for t, c in zip(tensors, batch_crops):
                    if literal:   # the reference's two calls
                        m.integrate_batch(_tta.d4_image_deaugment(t), c)
                    else:
                        m.integrate_batch_deaugment(t, c, group="d4", reduction="mean")
                return m.merge()

            try:
                for _ in range(3):
                    vstep()
                vr = sorted(timed_run(vstep, args.steps)[0] for _ in range(3))
                mode = m.mode
            finally:
                _tta.set_lazy_deaugment(prev[0])
                _tiles.set_auto_plan(prev[1])
                _tiles._auto.clear()
            del m
            return round(vr[1] / args.steps * 1e3, 4), mode

        mk = lambda **kw: (lambda: TileMerger(slicer.target_shape, CHANNELS, slicer.weight, device=dev, **kw))  # noqa: E731
        lit, lit_mode = variant(mk(), literal=True)
        lit_new, lit_new_mode = variant(mk(), literal=True, fresh=True)
        lit_inc, lit_inc_mode = variant(mk(), literal=True, self_plan=False)
        frac = lambda ms: round(region_bytes_all / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)  # noqa: E731
        # the model under torch.autocast: bfloat16 outputs (half the bytes in, the fp32 map out).  The literal calls hand the merger a lazy
        # handle of a HALF tensor; the fused launch rounds the reduced value to bfloat16 in registers (PTB_ROUND_SRC), as the eager pair does
        half_tensors = [t.to(torch.bfloat16) for t in batch_tensors]
        half_bytes = VIEWS * n_tiles * CHANNELS * TILE * TILE * 2 + CHANNELS * 5120 * 5120 * 4      # 6 476 005 376 B
        lit_bf16, lit_bf16_mode = variant(mk(), literal=True, fresh=True, tensors=half_tensors)
        ext_bf16 = variant(mk(crops=slicer.crops, defer=True, defer_rows=args.defer_rows or None), tensors=half_tensors)[0]
        del half_tensors
        variants = {
            "deferred_bands_ms": variant(mk(crops=slicer.crops, defer=True, defer_rows=args.defer_rows or None))[0],
            "deferred_one_band_per_launch_ms": variant(mk(crops=slicer.crops, defer=True, defer_rows=256))[0],
            "planned_no_defer_ms": variant(mk(crops=slicer.crops))[0],
            "unplanned_fused_ms": variant(mk(auto_plan=False))[0],
            "dropin_literal_ms": lit,
            "dropin_literal_merger_mode": lit_mode,
            "dropin_literal_hbm_frac": frac(lit),
            "dropin_literal_new_merger_per_image_ms": lit_new,
            "dropin_literal_new_merger_per_image_mode": lit_new_mode,
            "dropin_literal_new_merger_per_image_hbm_frac": frac(lit_new),
            "dropin_literal_no_self_planning_ms": lit_inc,
            "dropin_literal_no_self_planning_mode": lit_inc_mode,
            "dropin_literal_eager_ms": variant(mk(), literal=True, eager=True, self_plan=False)[0],
            "dropin_literal_bf16_ms": lit_bf16,
            "dropin_literal_bf16_mode": lit_bf16_mode,
            "dropin_literal_bf16_hbm_frac": round(half_bytes / (lit_bf16 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "deferred_bands_bf16_ms": ext_bf16,
            "deferred_bands_bf16_hbm_frac": round(half_bytes / (ext_bf16 * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "note": "ms per 5000x5000 image, median of 3 runs of K steps; deferred_bands = TileMerger(crops=, defer=True) + "
                    "integrate_batch_deaugment (the headline); planned_no_defer = TileMerger(crops=) + integrate_batch_deaugment; "
                    "unplanned_fused = TileMerger(auto_plan=False) + integrate_batch_deaugment + merge(); dropin_literal = the reference's "
                    "literal calls, no API extension, library defaults: TileMerger(shape, C, weight) + integrate_batch(tta.d4_image_deaugment(y), "
                    "crops) + merge() -- the de-augmentation comes back as a lazy handle the merger fuses into its launch, and from the second "
                    "image of a geometry on the merger plans itself into deferred bands from the crop sequence of the previous image (reset() per "
                    "image; _new_merger_per_image: a new TileMerger per image as in the README); _no_self_planning: tiles.set_auto_plan(False) "
                    "(round 4's default: lazy handle fused, accumulator in HBM, separate merge pass); dropin_literal_eager = "
                    "pytorch_toolbelt_amd.set_strict_dropin(): no lazy handles, no self-planning -- the reduced tile travels through HBM; "
                    "_hbm_frac = the region's 12 532 580 352 algorithmic bytes / ms / 8 TB/s; dropin_literal_bf16 = the literal calls (new merger per "
                    "image) on bfloat16 model outputs (torch.autocast), deferred_bands_bf16 = the headline's explicit form on the same tensors: "
                    "6 476 005 376 algorithmic bytes (half-precision views in, fp32 map out)",
        }

    if args.diag and rank == 0 and not use_dist:   # (extra steps on one rank only would leave the others' halo exchanges unmatched)
        per_step = []
        for _ in range(10):
            sync()
            t1 = time.perf_counter()
            step()
            th = time.perf_counter() - t1
            sync()
            per_step.append((round(th * 1e3, 3), round((time.perf_counter() - t1) * 1e3, 3)))
        depth = {}
        for k in (1, 2, 4, 8, 16, 32):
            sync()
            t1 = time.perf_counter()
            for _ in range(k):
                step()
            sync()
            depth[k] = round((time.perf_counter() - t1) * 1e3 / k, 3)
        print(f"[diag] ms/step for k unsynced steps: {depth}", file=sys.stderr)
        calls = []
        sync()
        for _ in range(3):
            merger.reset()
            for t, c in zip(batch_tensors, batch_crops):
                t1 = time.perf_counter()
                merger.integrate_batch_deaugment(t, c, group="d4", reduction="mean")
                calls.append((time.perf_counter() - t1) * 1e6)
            merger.merge()
        sync()
        calls = np.array(calls)
        print(f"[diag] cpus={os.cpu_count()} loadavg={os.getloadavg()} (host issue ms, step ms) per synced step: {per_step}", file=sys.stderr)
        print(f"[diag] integrate host us: min {calls.min():.1f} median {np.median(calls):.1f} p90 {np.percentile(calls, 90):.1f} max {calls.max():.1f}", file=sys.stderr)
        print(f"[diag] allocator: allocated {torch.cuda.memory_allocated() / 1e9:.2f} GB reserved {torch.cuda.memory_reserved() / 1e9:.2f} GB", file=sys.stderr)

    # ---- dominant-kernel roofline: ONE HIP-event pair (same stream) around the back-to-back run of full 8-tile launches
    # of a step (per-launch event pairs would insert a marker packet between kernels and inflate every launch by a few
    # microseconds); averaged over several steps.  The trailing partial batch and the merge are outside the bracket.  --full only, like
    # the box's read ceiling and the placement search below.
    if args.full:
        n_full = sum(1 for c in batch_crops if len(c) == BATCH)
        assert all(len(c) == BATCH for c in batch_crops[:n_full])
        spans = []
        for _ in range(max(3, min(10, args.steps))):
            merger.reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for t, c in zip(batch_tensors[:n_full], batch_crops[:n_full]):
                merger.integrate_batch_deaugment(t, c, group="d4", reduction="mean")
            e1.record()
            for t, c in zip(batch_tensors[n_full:], batch_crops[n_full:]):
                merger.integrate_batch_deaugment(t, c, group="d4", reduction="mean")
            merger.merge()
            torch.cuda.synchronize()
            spans.append(e0.elapsed_time(e1))
        launch_ms = float(np.median(spans)) / max(n_full, 1) if n_full else float("nan")
        bytes_per_tile = VIEWS * CHANNELS * TILE * TILE * 4          # 8 views x C x T x 4 B read per tile
        bytes_per_launch = bytes_per_tile * BATCH
        n_bands = len(merger._bands.bands) if (not sharded and deferred) else 0
        if n_bands:
            # deferred: the band-group launches of an image ARE the region (they read every model output once and write the merged
            # map once) and nothing else runs on the stream: one HIP-event pair around the K timed steps / (K x launches per image)
            launch_ms = region_event_ms / (args.steps * n_bands)
            bytes_per_launch = (VIEWS * n_tiles * CHANNELS * TILE * TILE * 4 + CHANNELS * 5120 * 5120 * 4) // n_bands
        elif sharded:
            # one rank's share of the image: its tiles read once + its owned rows written once, over the whole step (kernels, the
            # partial-sum exchange and the completion of the shared rows) -- the per-rank effective rate, not a single kernel's
            owned = merger.owned_rows or (0, 0)
            bytes_per_launch = bytes_per_tile * len(crops) + CHANNELS * (owned[1] - owned[0]) * 5120 * 4
            launch_ms = elapsed / args.steps * 1e3
        elif not sharded and planned:
            # the planned kernel also writes the region's output (+ C x 5120 x 5120 x 4 B per image): the launch's
            # share of the whole region's algorithmic bytes, 12 532 580 352 B x 8 / 361
            bytes_per_launch += CHANNELS * 5120 * 5120 * 4 * BATCH // n_tiles
        achieved = bytes_per_launch / (launch_ms * 1e-3) / 1e9

    # ---- what this box's memory system gives a pure read stream over the same buffers (boxes of one pool differ by ~10 %)
    box_ceiling = None
    if args.full and not use_dist:
        sink = torch.zeros(4, device=dev)
        lib = N.load()

        import ctypes

        nb = len(batch_tensors)
        ptrs = (ctypes.c_void_p * nb)(*[t.data_ptr() for t in batch_tensors])
        sizes = (ctypes.c_int64 * nb)(*[t.numel() * t.element_size() for t in batch_tensors])

        def probe_pass(wgs):   # ONE launch over all batches (a persistent grid; ramp-up and tail paid once, like a band launch)
            got = lib.ptb_read_probe_multi(ptrs, sizes, nb, sink.data_ptr(), wgs, N.stream_ptr(dev))
            assert got > 0, got
            return got

        best = 0.0
        for wgs in (2048, 4096, 8192):
            probe_pass(wgs)
            torch.cuda.synchronize()
            pe0, pe1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            pe0.record()
            read = sum(probe_pass(wgs) for _ in range(3))
            pe1.record()
            torch.cuda.synchronize()
            best = max(best, read / (pe0.elapsed_time(pe1) * 1e-3) / 1e9)
        box_ceiling = best

    # ---- placement of the model outputs (reported, NOT the headline).  Where the 12 GB of model outputs sit in device memory decides
    # up to 10-15 % of this loop's speed on some boxes.  `value` above is measured on the pool exactly as torch's
    # allocator first handed it out -- what a user of the library gets.  What a process that owns its buffer pool could get by
    # choosing among candidate pools at start-up (pytorch_toolbelt_amd/placement.py) is measured here, afterwards, as
    # config.best_placement: candidate pools are allocated one ~36 GB region apart, a few steps are run on each, the fastest is
    # kept and timed with the same K steps.  --placement-tries 1 skips it.
    placement = {"max_tries": 1, "ms_per_step_by_candidate": [], "chosen": 0} if args.full else None
    best_placement = None
    if args.full and args.placement_tries > 1 and not use_dist:
        search_steps = 0

        def run_ms(tensors, k):
            nonlocal batch_tensors, search_steps
            search_steps += k + 1
            batch_tensors = tensors                      # (step() reads the variable)
            q0, q1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            step()
            q0.record()
            for _ in range(k):
                step()
            q1.record()
            torch.cuda.synchronize()
            return q0.elapsed_time(q1) / k

        from pytorch_toolbelt_amd.placement import choose_placement

        need = sum(t.numel() * t.element_size() for t in batch_tensors)
        (batch_tensors, _keep), rep = choose_placement(
            lambda: alloc_outputs(0), lambda pool: min(run_ms(pool[0], 4), run_ms(pool[0], 4)), need, dev, first=(batch_tensors, _keep),
            max_tries=args.placement_tries)
        per_cand, chosen = rep["by_candidate"], rep["chosen"]
        torch.cuda.empty_cache()      # (the first pool was still referenced from here while the search ran)
        placement = {"max_tries": args.placement_tries, "ms_per_step_by_candidate": per_cand, "chosen": chosen, "steps_run_by_the_search": search_steps,
                     "steps_after_the_headline": search_steps + 10 + 3 * args.steps,   # (for tools/profile_report.py: search + best-placement timing)
                     "note": "AFTER the headline was measured: candidate pools for the model outputs are allocated side by side, a few steps are "
                             "run on each, the fastest is kept and timed (config.best_placement)"}
        for _ in range(10):
            step()
        bp = sorted(timed_run(step, args.steps)[0] for _ in range(3))[1] / args.steps * 1e3
        best_placement = {"ms_per_step": round(bp, 4), "value_MP_s": round(IMAGE[0] * IMAGE[1] / 1e3 / bp, 1),
                          "region_hbm_frac": round((VIEWS * n_tiles * CHANNELS * TILE * TILE * 4 + CHANNELS * 5120 * 5120 * 4) / (bp * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                          "note": "the same K steps (median of 3 runs) on the fastest of the candidate pools -- an upper envelope for callers that own "
                                  "their allocation; NOT `value`"}

    mp = IMAGE[0] * IMAGE[1] / 1e6
    ms_per_step = elapsed / args.steps * 1e3
    value = mp * args.steps / elapsed  # one image per step for the whole job (strong scaling for N > 1)
    region_bytes = VIEWS * n_tiles * CHANNELS * TILE * TILE * 4 + CHANNELS * 5120 * 5120 * 4  # 12 532 580 352 B

    traffic, traffic_when = None, ""
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    if args.full and os.path.exists(tpath):
        try:
            tj = json.load(open(tpath))
            traffic = tj.get("band_plan_d4_bytes_per_launch" if n_bands else "view_accum_d4_bytes_per_launch")
            if tj.get("measured"):
                traffic_when = f"; PMC run of {tj['measured']}"
        except Exception:
            traffic = None

    if rank == 0:
        line = {
            "metric": "megapixels/sec tiled+d4-TTA merge on 5000x5000",
            "value": round(value, 1),
            "unit": "MP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "strong",  # one image per step for the whole job, whatever N
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": "BASELINE cfg2: 5000x5000x3 image, ImageSlicer 512/256 pyramid (361 tiles, target 5120x5120), "
                            "d4 TTA (8 views) model outputs C=4 fp32 resident in HBM, fused de-augment+mean+integrate_batch in "
                            "batches of 8 tiles + merge; accumulators reset (first-touch stores, no memset) each step; " +
                            ("TileMerger(crops=tiler.crops, defer=True): the merger keeps references to the (resident, unmodified) "
                             "batches; the data-independent norm_mask is precomputed from the crop list (SURVEY 8d: not compulsory "
                             f"traffic); each group of bands ({merger._bands.bands[0][1] - merger._bands.bands[0][0]} rows) of the image is merged by ONE "
                             f"launch when its last tile has arrived ({len(merger._bands.bands)} launches per image, planned once and driven "
                             "from C: ptb_band_plan_submit; no accumulator in HBM), so merge() returns the finished [C,H',W'] map; "
                             if (not sharded and deferred) else
                             "TileMerger(crops=tiler.crops): the data-independent norm_mask is precomputed from the crop list (SURVEY 8d: "
                             "not compulsory traffic) and every block is divided by it in the launch that brings its last tile, so "
                             "merge() returns the finished [C,H',W'] map; " if (not sharded and planned) else
                             ("ShardedTileMerger: every rank merges its tiles band by band straight from the model outputs (C band plan, no "
                              "accumulator; rows shared with a neighbour hold partial sums), the partial-sum rectangles go point-to-point to "
                              "the rank owning those rows, each rank adds what it received and divides those rows by the locally computed "
                              "norm_mask; " if sharded
                              else "norm_mask built lazily from the crop log, merge() = one division pass; ")) +
                            "model forward excluded",
                "tiles": n_tiles,
                "batch_tiles": BATCH,
                "merger": ("planned + deferred bands (crops= given, defer=True)" if (not sharded and deferred) else
                           "planned (crops= given, no merge pass)" if (not sharded and planned) else
                           (("sharded, deferred bands" if getattr(merger, "_deferred", None) is not None else "sharded, incremental") if sharded
                            else "unplanned (lazy norm_mask + merge pass)")),
                "parallelism": "single GPU" if world == 1 else (f"{'tile ranges' if partition == 'tiles' else 'tile rows'} sharded over {world} ranks, RCCL p2p halo exchange"),
                "model_outputs": ("slices of one 12.1 GB tensor" if os.environ.get("PTB_BENCH_ONE_BUFFER", "0") == "1" else
                                  "one tensor per batch" + (", carved by torch's caching allocator out of ONE device allocation reserved up front "
                                                            "(PTB_BENCH_PRIME_POOL=0: 46 separate 256 MiB device allocations)"
                                                            if os.environ.get("PTB_BENCH_PRIME_POOL", "1") == "1" else ", 46 separate device allocations")),
                "placement": placement,
                "first_allocation": {"ms_per_step": round(ms_per_step, 4), "value_MP_s": round(value, 1),
                                     "region_hbm_frac": round(region_bytes / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS, 4),
                                     "note": "`value` IS the first-allocation figure: the model-output pool as torch's allocator first handed it out"},
                "best_placement": best_placement,
                "fallback": fallback,
                "parity": parity1,
                "dropin_literal": None if variants is None else {
                    "ms_per_step": variants["dropin_literal_new_merger_per_image_ms"],
                    "value_MP_s": round(IMAGE[0] * IMAGE[1] / 1e3 / variants["dropin_literal_new_merger_per_image_ms"], 1),
                    "region_hbm_frac": variants["dropin_literal_new_merger_per_image_hbm_frac"],
                    "merger_mode": variants["dropin_literal_new_merger_per_image_mode"],
                    "note": "the reference's loop verbatim on this library's defaults (README.md:201-226: a new TileMerger(shape, C, weight) per "
                            "image, integrate_batch(tta.d4_image_deaugment(y), crops), merge()) -- no crops=, no defer=, no "
                            "integrate_batch_deaugment; `value` above is the same kernels reached through the explicit extensions"},
                "host_issue_ms_per_step": round(host_ms, 4),
                "timing": f"value = median of {len(repeat_ms)} runs of exactly {args.steps} steps, each bracketed by barrier + synchronize",
                "repeat_ms_per_step": repeat_ms,
                "repeat_min_median_max_ms": [min(repeat_ms), sorted(repeat_ms)[len(repeat_ms) // 2], max(repeat_ms)],
                "ramp_ms_per_step_groups_of_10": [round(v, 3) for v in ramp_groups],
                "variants": variants,
                "sharded": sharded_report,
                "region_algorithmic_bytes": region_bytes,
                "region_hbm_frac": round(region_bytes / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS, 4),
            },
            "roofline": {
                "kernel": ("band_plan_kernel<8,D4,linear> (fused d4 de-augment + mean + weighted blend of all covering tiles + "
                           f"normalisation over one group of bands; {n_bands} launches/image)" if n_bands else
                           ("rank 0's whole step (band_plan_kernel launches over its tiles + partial-sum exchange + completion of the rows "
                            "shared with neighbours): its tiles read once and its owned rows written once / step time" if sharded else
                            "view_accum_kernel<CH,8,D4,linear> (fused d4 de-augment + mean + weighted accumulate + last-touch "
                            "normalisation, 8 tiles/launch)")),
                "bound": "hbm",
                "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": traffic,
                "traffic_source": "rocprofv3 PMC passes of this command (profiles/traffic.json: FETCH_SIZE x2 + WRITE_SIZE per launch), not re-measured in "
                                  "this run" + traffic_when,
                "box_read_ceiling": None if box_ceiling is None else round(box_ceiling, 1),
                "frac_of_box_read_ceiling": None if box_ceiling is None else round(achieved / box_ceiling, 4),
                "box_read_ceiling_note": "GB/s of a pure read-only stream (ptb_read_probe_multi: 16 B/lane, 8 nt loads in flight, ONE launch of a "
                                         "persistent grid over all batches, best of 2048 / 4096 / 8192 workgroups) over the same 12.1 GB of model "
                                         "outputs on THIS box, measured in this run",
                "algorithmic_bytes_per_launch": bytes_per_launch,
                "avg_launch_ms": round(launch_ms, 5),
            } if args.full else None,
        }
        if args.full and world == 1 and not use_dist and not args.no_secondary:     # (before the CPU baseline: the GPU is still at its clocks)
            del batch_tensors, _keep
            torch.cuda.empty_cache()
            try:
                line["config"]["secondary"] = secondary_workloads(dev, with_cpu=not args.no_cpu_baseline)
            except Exception as exc:  # noqa: BLE001  (the headline line must survive a failing side measurement)
                line["config"]["secondary"] = {"error": repr(exc)}
        if args.full and world == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(slicer)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # RCCL writes its version banner through C stdio, which would otherwise be flushed AFTER this line at exit:
        # flush it first so the JSON line is the last thing on stdout
        import ctypes

        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(json.dumps(line), flush=True)
    if parity1 is not None and not parity1["max_abs_diff_vs_plain_merger"] <= parity1["tolerance"]:
        print(f"[bench] the timed merger's output differs from the plain merger's by {parity1['max_abs_diff_vs_plain_merger']:.3g}: the timing above is not a "
              "valid result", file=sys.stderr, flush=True)
        sys.exit(3)
    if parity is not None and not parity["parity_max_abs_diff"] <= parity["parity_tolerance"]:
        print(f"[bench] rank {rank}: the sharded merge differs from the single-device merge by {parity['parity_max_abs_diff']:.3g} "
              f"(tolerance {parity['parity_tolerance']}): the timing above is not a valid result", file=sys.stderr, flush=True)
        sys.exit(3)


if __name__ == "__main__":
    main()
