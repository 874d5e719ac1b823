#!/usr/bin/env python3
"""Which kernel does every call of the C ABI launch?  Without a GPU: tools/dispatch_probe_shim.cpp defines the few HIP entry points
libptb_hip.so imports (kernel registration, the launch, memset / memcpy), so a launch only writes the kernel's name, grid, block and
LDS bytes to a log.  This script calls the entry points over the arguments their launch sites dispatch on -- class counts on both
sides of the register buckets, HW eligible or not for the straight-line kernels, aligned or not, labels or dense targets, every
reduction, view set, source type, crop kind, tunable -- with made-up device pointers that nothing dereferences.

    python tools/dispatch_probe.py path/to/libptb_hip.so out.log

Two builds of the library select the same instance for every call exactly when the launch lines of their logs (``grep -v '^#'``)
are equal; ``sort -u`` of the first column against tools/kernel_manifest.py's names gives the kernels no call here reaches."""
import ctypes as C, itertools as it, os, subprocess, sys, tempfile
lib_path, log = sys.argv[1], sys.argv[2]
_tmp = tempfile.mkdtemp()
_shim = os.path.join(_tmp, "shim.so")
subprocess.run(["g++", "-O1", "-shared", "-fPIC", os.path.join(os.path.dirname(os.path.abspath(__file__)), "dispatch_probe_shim.cpp"), "-o", _shim], check=True)
shim = C.CDLL(_shim, mode=C.RTLD_GLOBAL)   # loaded first and globally: the library's HIP imports bind to it
L = C.CDLL(lib_path)
shim.ptb_shim_open(log.encode())
P = 0x7f0000000000            # fake device pointers: 16-byte aligned, and one that is not
def p(k, off=0): return C.c_void_p(P + (k << 32) + off)
NUL = C.c_void_p(0)
i64, f32, f64, i32 = C.c_int64, C.c_float, C.c_double, C.c_int
def call(name, *a):
    shim.ptb_shim_mark((name + " " + " ".join(str(getattr(x, "value", x)) for x in a)).encode())
    rc = getattr(L, name)(*a)
    shim.ptb_shim_mark(("rc %d" % rc).encode())
def arr(t, v): return (t * len(v))(*v)
n = 0
for scalar in (0, 1):
    L.ptb_set_tunable(1, scalar)
    for Cc, HW, un in it.product((1, 3, 4, 5, 8, 9, 16, 17), (252, 256, 1024, 1280, 384), (0, 4)):
        for flags, prob, gamma, lab, cw in it.product((1, 2, 3, 3 | 4, 3 | 8, 3 | 16, 3 | 64, 3 | 128, 1 | 128, 1 | 4, 2 | 4, 1 | 64), (0, 1, 2), (2.0, 1.5), (0, 1), (0, 1)):
            labels, dense = (p(2), NUL) if lab else (NUL, p(3))
            cwp = p(4) if cw else NUL
            call("ptb_seg_loss_fwd", p(1, un), labels, dense, cwp, p(5), p(6), p(7), i32(2), i32(Cc), i64(HW), i32(flags), i32(prob), f32(gamma), f32(0.25), f32(0.5), i64(255), f32(255.0), NUL)
            if flags & 1 and not flags & 2:
                for ge in (NUL, p(8)):
                    call("ptb_focal_bwd", p(1, un), labels, dense, cwp, p(5), ge, p(6), i32(2), i32(Cc), i64(HW), i32(flags), f32(gamma), f32(0.25), f32(0.5), i64(255), f32(255.0), NUL)
            if flags & 2:
                call("ptb_seg_stats_bwd", p(1, un), labels, dense, p(5), p(6), p(7), i32(2), i32(Cc), i64(HW), i32(flags), i32(prob), i64(255), f32(255.0), NUL)
            if (flags & 3) == 3:
                call("ptb_seg_fused_bwd", p(1, un), labels, dense, cwp, p(5), p(6), p(7), p(8), i32(2), i32(Cc), i64(HW), i32(flags), i32(prob), f32(gamma), f32(0.25), f32(0.5), i64(255), f32(255.0), NUL)
        for red, gamma, cw in it.product((0, 1), (2.0, 1.0), (0, 1)):
            cwp = p(4) if cw else NUL
            call("ptb_softmax_focal_fwd", p(1, un), p(2), cwp, p(5), p(6), p(7), i32(2), i32(Cc), i64(HW), i32(red), f32(gamma), f32(0.5), i64(-100), NUL)
            for stash in (0, 2, 4):
                L.ptb_set_tunable(7, stash)
                call("ptb_softmax_focal_bwd", p(1, un), p(2), cwp, p(5), p(6), p(7), i32(2), i32(Cc), i64(HW), i32(red), f32(gamma), f32(0.5), i64(-100), NUL)
            L.ptb_set_tunable(7, 0)
            call("ptb_focal_softmax_fwd", p(1, un), p(2), NUL, NUL, i32(0), i32(0), i64(1), p(5), p(6), p(7), i32(2), i32(Cc), i64(HW), i32(1), f32(gamma), f32(0.25), f32(0.5), i64(255), f32(255.0), NUL)
        call("ptb_soft_ce_fwd", p(1, un), p(2), p(5), p(6), p(7), i32(2), i32(Cc), i64(HW), f32(0.1), i32(0), i64(-100), NUL)
        call("ptb_soft_ce_bwd", p(1, un), p(2), p(5), p(6), p(7), i32(2), i32(Cc), i64(HW), f32(0.1), i32(0), i64(-100), NUL)
        ins = arr(C.c_void_p, [P + (20 + t << 32) + un for t in range(3)])
        for red, act in it.product(range(7), (0, 1, 2)):
            call("ptb_ensemble_reduce", ins, i32(3), i32(red), i32(act), f32(1.0), i32(2), i32(Cc), i64(HW), p(6), NUL)
    for kind, nn, un, emit in it.product(range(6), (1024, 1023), (0, 4), (0, 1)):
        call("ptb_pointwise_loss_fwd", i32(kind), p(1, un), p(2), NUL, NUL, p(5), p(6), i64(nn), i32(1), i64(nn), i32(0), f32(1), f32(1), f32(1), f32(255), NUL)
        call("ptb_pointwise_loss_apply", i32(kind), i32(emit), p(1, un), p(2), NUL, NUL, p(5), NUL, p(6), i64(nn), i32(1), i64(nn), i32(0), f32(1), f32(1), f32(1), f32(255), NUL)
    for red, nn, un in it.product(range(7), (1024, 1023), (0, 4)):
        call("ptb_stack_reduce", p(1, un), i32(3), i64(nn), i32(red), f64(1e-6), p(6), NUL)
        call("ptb_stack_reduce_bwd", p(1, un), p(2), p(3), i32(3), i64(nn), i32(red), f64(1e-6), p(6), NUL)
    for kind, Cc, layout, W in it.product(range(6), (1, 2, 3, 4, 5), (0, 1), (64, 63)):
        call("ptb_volume_merge_crop", p(1), p(2), i32(Cc), i32(8), i32(32), i32(W), i32(0), i32(4), i32(4), i32(8), i32(16), i32(W - 8), i32(layout), i32(kind), p(6), NUL)
        if kind < 4:
            call("ptb_merge_crop", p(1), p(2), i32(Cc), i32(32), i32(W), i32(4), i32(4), i32(16), i32(W - 8), i32(layout), i32(kind), p(6), NUL)
    for cl, dt, red, W, nv in it.product((0, 0x200), (0, 1, 2), range(7), (8, 7), (1, 2, 8)):
        masks = arr(i32, list(range(nv)))
        call("ptb_volume_mirror_reduce", p(1), i32(dt | cl), p(6), i32(nv), masks, i32(red), i32(2), i32(4), i32(8), i32(8), i32(W), NUL)
        z = arr(i64, [0, 8]); y = arr(i64, [0, 4]); x = arr(i64, [0, 3])
        call("ptb_volume_mirror_accumulate", p(1), p(2), p(3), p(4), i32(dt | cl), i32(nv), masks, i32(red), z, y, x, i32(2), i32(4), i32(8), i32(8), i32(W), i32(16), i32(16), i32(16), NUL)
        if red < 2 and not cl:
            call("ptb_volume_mirror", p(1), i32(dt), p(6), i32(nv), masks, i32(red), i32(2), i32(4), i32(8), i32(8), i32(W), NUL)
    VIEWS = {"id": [0], "fliplr": [0, 4], "flipud": [0, 2], "flips": [0, 4, 2], "d2": [0, 4, 2, 6], "d4": [0, 5, 6, 3, 1, 4, 7, 2], "other": [0, 1, 3], "two": [4, 0]}
    for ch in (16, 32, 64):
        L.ptb_set_tunable(0, ch)
        for (vn, v), dt, red, W, cl in it.product(VIEWS.items(), (0, 1, 2), (0, 1, 2, 5), (32, 30), (0, 0x200, 0x100, 0x300)):
            views = arr(i32, v)
            call("ptb_deaug_reduce_t", p(1), i32(dt | cl), p(6), i32(len(v)), views, i32(red), i32(2), i32(3), i32(W), i32(W), NUL)
            xs = arr(i64, [0, 16]); ys = arr(i64, [0, 16])
            call("ptb_deaug_accumulate_t", p(6), p(7), p(8), p(1), i32(dt | cl), i32(len(v)), views, i32(red), xs, ys, i32(2), i32(3), i32(W), i32(W), i32(64), i32(64), NUL, i32(0), NUL)
        for ind, outd, W, v in it.product((3, 4, 5), (0, 1, 2), (32, 30), ([0], [0, 4], [0, 1])):
            xs = arr(i64, [0, 16]); ys = arr(i64, [-4, 16])
            call("ptb_split_tiles", p(1), i32(ind), i32(64), i32(64), i32(3), xs, ys, i32(2), i32(W), i32(W), i32(len(v)), arr(i32, v), NUL, NUL, i32(0), f32(0), i32(outd), p(6), NUL)
    L.ptb_set_tunable(0, 32)
    for ind, outd, w, nv in it.product(range(6), (0, 1, 2), (8, 7), (1, 2)):
        z = arr(i64, [0, 4]); y = arr(i64, [0, 4]); x = arr(i64, [-2, 4])
        call("ptb_volume_split_mirror", p(1), i32(ind), i32(16), i32(16), i32(16), i32(2), z, y, x, i32(2), i32(8), i32(8), i32(w), NUL, NUL, f32(0), i32(nv), arr(i32, list(range(nv))), i32(outd), p(6), NUL)
    for tw, tr in ((128, 32), (64, 16), (64, 32), (64, 64)):
        L.ptb_set_tunable(15, tw); L.ptb_set_tunable(6, tr)
        for V, inner, outer, al, sz in it.product((1, 2, 3, 4), (1, 2, 3), (0, 1, 2, 4), (0, 1), ((256, 256), (200, 250))):
            ins = arr(C.c_void_p, [P + (30 + t << 32) for t in range(2)])
            hs = arr(i32, [sz[0], sz[0] // 2]); ws = arr(i32, [sz[1], sz[1] // 2])
            call("ptb_ms_flip_deaug_reduce", ins, hs, ws, i32(2), i32(V), arr(i32, [0, 4, 2, 6][:V]), i32(inner), p(6), i64(3), i32(sz[0]), i32(sz[1]), i32(al), i32(outer), NUL)
    L.ptb_set_tunable(15, 128); L.ptb_set_tunable(6, 32)

    # deferred merges: one band (ptb_merge_band), the band plan and the volume plan
    L.ptb_band_plan_create.restype = C.c_int64; L.ptb_volume_plan_create.restype = C.c_int64
    xs = arr(i64, [0, 16, 0, 16]); ys = arr(i64, [0, 0, 16, 16])
    for (vn, v), dt, red, cl in it.product(VIEWS.items(), (0, 1, 2), (0, 1, 2, 5), (0, 0x200)):
        V = len(v)
        src = arr(C.c_void_p, [P + (40 + t << 32) for t in range(4)]); vs = arr(i64, [4 * 3 * 32 * 32] * 4)
        call("ptb_merge_band", p(6), p(7), p(8), src, vs, i32(dt | cl), i32(V), arr(i32, v), i32(red), xs, ys, i32(4), i32(3), i32(32), i32(32), i32(48), i32(48), i32(16), i32(32), NUL)
        for rows, pf in it.product((32, 64), (0, 1, 2)):
            L.ptb_set_tunable(11, rows); L.ptb_set_tunable(21, pf)
            plan = C.c_void_p()
            nb = L.ptb_band_plan_create(xs, ys, i32(4), i32(3), i32(32), i32(32), i32(48), i32(48), i32(1024), i32(0), i32(48), NUL, i32(0), C.byref(plan))
            shim.ptb_shim_mark(("plan %d rows %d pf %d" % (nb, rows, pf)).encode())
            if nb >= 0 and plan:
                call("ptb_band_plan_upload", plan, p(9), NUL)
                call("ptb_band_plan_submit", plan, i32(0), i32(4), p(1), i64(3 * 32 * 32), i64(4 * 3 * 32 * 32), i32(dt | cl), i32(V), arr(i32, v), i32(red), p(6), p(7), p(8), NUL)
                L.ptb_band_plan_destroy(plan)
        L.ptb_set_tunable(11, 64); L.ptb_set_tunable(21, 1)
    z = arr(i64, [0, 0, 4, 4]); y = arr(i64, [0, 4, 0, 4]); x = arr(i64, [0, 0, 0, 0])
    for kind, layout, dt, cl, nv, red, w in it.product(range(6), (0, 1), (0, 1, 2), (0, 0x200), (0, 1, 2), (1, 2), (8, 6)):
        plan = C.c_void_p()
        nb = L.ptb_volume_plan_create(z, y, x, i32(4), i32(4), i32(8), i32(8), i32(w), i32(12), i32(12), i32(w), arr(i64, [0, 0, 0, 12, 12, w]), i32(layout), i32(kind), C.byref(plan))
        shim.ptb_shim_mark(("volume plan %d" % nb).encode())
        if nb >= 0 and plan:
            call("ptb_volume_plan_upload", plan, p(9), NUL)
            call("ptb_volume_plan_submit", plan, i32(0), i32(4), p(1), i64(4 * 8 * 8 * w), i64(4 * 4 * 8 * 8 * w), i32(dt | cl), i32(nv), arr(i32, list(range(nv))), i32(red), p(8), p(6), NUL)
            L.ptb_volume_plan_destroy(plan)
    # the activations of ptb_volume_activation.hip: softmax on both sides of the 8 channels of the 4-voxel lanes, sigmoid beyond 16
    for (act, Cc), dt, cl, W, nv in it.product(((2, 4), (2, 8), (2, 9), (2, 16), (1, 3), (1, 20), (0, 4)), (0, 1, 2), (0, 0x200), (8, 7), (1, 8)):
        masks = arr(i32, list(range(nv)))
        call("ptb_volume_mirror_reduce_act", p(1), i32(dt | cl), p(6), i32(nv), masks, i32(2), i32(2), i32(Cc), i32(8), i32(8), i32(W), i32(act), f32(1.0), NUL)
        z = arr(i64, [0, 8]); y = arr(i64, [0, 4]); x = arr(i64, [0, 3])
        call("ptb_volume_mirror_accumulate_act", p(1), p(2), p(3), p(4), i32(dt | cl), i32(nv), masks, i32(2), z, y, x, i32(2), i32(Cc), i32(8), i32(8), i32(W), i32(16), i32(16), i32(16), i32(act), f32(1.0), NUL)
    z = arr(i64, [0, 0, 4, 4]); y = arr(i64, [0, 4, 0, 4]); x = arr(i64, [0, 0, 0, 0])
    for kind, dt, cl, nv, w, (act, Cc) in it.product(range(6), (0, 1, 2), (0, 0x200), (0, 8), (8, 6), ((2, 4), (2, 9), (1, 20))):
        plan = C.c_void_p()
        nb = L.ptb_volume_plan_create(z, y, x, i32(4), i32(Cc), i32(8), i32(8), i32(w), i32(12), i32(12), i32(w), arr(i64, [0, 0, 0, 12, 12, w]), i32(0), i32(kind), C.byref(plan))
        shim.ptb_shim_mark(("volume plan %d" % nb).encode())
        if nb >= 0 and plan:
            call("ptb_volume_plan_upload", plan, p(9), NUL)
            call("ptb_volume_plan_submit_act", plan, i32(0), i32(4), p(1), i64(Cc * 8 * 8 * w), i64(4 * Cc * 8 * 8 * w), i32(dt | cl), i32(nv), arr(i32, list(range(nv))), i32(2), p(8), p(6), i32(act), f32(1.0), NUL)
            L.ptb_volume_plan_destroy(plan)
    # the activations of ptb_tile_activation.hip: every view set, source type and layout, on and off the 4-pixel grid, at the three chunk
    # sizes; softmax on both sides of 16 channels, sigmoid beyond them
    L.ptb_band_plan_submit_act.restype = C.c_int
    for ch in (16, 32, 64):
        L.ptb_set_tunable(0, ch)
        for (vn, v), dt, W, cl, (act, Cc) in it.product(VIEWS.items(), (0, 1, 2), (32, 30), (0, 0x200), ((2, 3), (2, 16), (2, 17), (1, 20), (0, 4))):
            views = arr(i32, v)
            call("ptb_deaug_reduce_act", p(1), i32(dt | cl), p(6), i32(len(v)), views, i32(2), i32(2), i32(Cc), i32(W), i32(W), i32(act), f32(1.0), NUL)
            xs = arr(i64, [0, 16]); ys = arr(i64, [0, 16])
            call("ptb_deaug_accumulate_act", p(6), p(7), p(8), p(1), i32(dt | cl), i32(len(v)), views, i32(2), xs, ys, i32(2), i32(Cc), i32(W), i32(W), i32(64), i32(64), NUL, i32(0), i32(act), f32(1.0), NUL)
    L.ptb_set_tunable(0, 32)
    xs = arr(i64, [0, 16, 0, 16]); ys = arr(i64, [0, 0, 16, 16])
    for (vn, v), dt, cl, rows, (act, Cc) in it.product(VIEWS.items(), (0, 1, 2), (0, 0x200), (32, 64), ((2, 3), (2, 17), (1, 20))):
        L.ptb_set_tunable(11, rows)
        plan = C.c_void_p()
        nb = L.ptb_band_plan_create(xs, ys, i32(4), i32(Cc), i32(32), i32(32), i32(48), i32(48), i32(1024), i32(0), i32(48), NUL, i32(0), C.byref(plan))
        shim.ptb_shim_mark(("plan %d rows %d" % (nb, rows)).encode())
        if nb >= 0 and plan:
            call("ptb_band_plan_upload", plan, p(9), NUL)
            call("ptb_band_plan_submit_act", plan, i32(0), i32(4), p(1), i64(Cc * 32 * 32), i64(4 * Cc * 32 * 32), i32(dt | cl), i32(len(v)), arr(i32, v), i32(2), p(6), p(7), p(8), i32(act), f32(1.0), NUL)
            L.ptb_band_plan_destroy(plan)
    L.ptb_set_tunable(11, 64)
L.ptb_set_tunable(1, 0)
shim.ptb_shim_close()
