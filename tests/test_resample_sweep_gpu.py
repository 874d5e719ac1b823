"""GPU sweep of csrc/ptb_resample.hip against the float64 operator model of oracle/resample_oracle.py: the five resize kernels and their
atomic adjoints at ratios from 1/3 to 70, the three bilinear multiscale-merge kernels at every output width mod 4, the acceptance
boundary of the fused flips + multiscale kernel for all six tile shapes, the merge's backward, and the nearest-exact ties.

Tolerances: nearest modes are gathers -- bit-exact.  Linear arithmetic (bilinear / bicubic / area forward, sum and mean merges): with d
the largest deviation of the float32 numpy restatement (oracle.tta_oracle) from the float64 model on the same inputs, the kernel stays
within 4 d + 1e-7 (FMA contraction, another summation order).  Non-linear merges (hardware log / exp): rtol = atol = 1e-5.  Atomic
adjoints and the merge's backward: rtol = 2e-4, atol = 2e-5, as the golden gradient tests."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_cases as RC
from oracle import resample_oracle as RO
from oracle import tta_oracle as AO

pytestmark = pytest.mark.gpu

TUNABLE_DEFAULTS = {1: 0, 3: 1, 6: 32, 15: 128}      # force-scalar, tiled multiscale merge, fused tile rows, fused tile width
VIEWS = {"ident": (0,), "fliplr": (0, 4), "flipud": (0, 2), "d2": (0, 4, 2, 6)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def native():
    from pytorch_toolbelt_amd import _native as N

    lib = N.load()
    yield N
    for key, value in TUNABLE_DEFAULTS.items():
        lib.ptb_set_tunable(key, value)


@contextlib.contextmanager
def tunables(lib, **values):
    """ptb_set_tunable(key, value) for ``k<key>=value`` arguments; the defaults come back whatever happens inside."""
    try:
        for name, value in values.items():
            assert lib.ptb_set_tunable(int(name[1:]), value) == 0
        yield
    finally:
        for key, value in TUNABLE_DEFAULTS.items():
            lib.ptb_set_tunable(key, value)


def _tta():
    from pytorch_toolbelt_amd.inference import tta

    return tta


def _resample():
    from pytorch_toolbelt_amd.inference import _resample

    return _resample


def _worst(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max())


def _close(got, ref, rtol, atol):
    return bool(np.all(np.abs(got.astype(np.float64) - ref) <= atol + rtol * np.abs(ref)))


# ------------------------------------------------------------------------------------------------- A. single resizes
def _check_resize(native, dev, mode, ac, planes, src, size, seed):
    x = RC.uniform(planes + src, seed)
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    before = native.calls
    y = _resample().resize(xt, size, mode, ac)
    got = y.detach().cpu().numpy()
    model = RO.resize(x, size, mode, ac)
    assert got.shape == model.shape and got.dtype == np.float32
    if mode in ("nearest", "nearest-exact"):
        assert np.array_equal(got, model.astype(np.float32))
        d = 0.0
    else:
        d = _worst(RC.restated_resize_f32(x, size, mode, ac), model)
        err = _worst(got, model)
        print(f"{mode} ac={ac} {src}->{size}: restatement d = {d:.3g}, kernel {err:.3g}")
        assert err <= 4 * d + 1e-7
    g = RC.grad_weights(got.shape)
    (y * torch.from_numpy(g).to(dev)).sum().backward()
    assert native.calls == before + 2
    np.testing.assert_allclose(xt.grad.cpu().numpy(), RO.resize_adjoint(g, src, mode, ac), rtol=2e-4, atol=2e-5)
    return d


@pytest.mark.parametrize("shape", RC.SHAPES, ids=RC.SHAPE_IDS)
@pytest.mark.parametrize("mode,ac", RC.MODE_CASES, ids=RC.MODE_IDS)
def test_single_resize_and_adjoint(mode, ac, shape, dev, native):
    """Forward and backward of _resample.resize on 2 x 3 planes: 1-pixel inputs and outputs (align_corners with an output extent of 1:
    scale 0), ratios 3 and 1 / 3 (3 x 3 area windows; bicubic taps clamped on both sides at 5 x 7 and 2 x 3), odd ratios, a 257-wide
    output (scalar stores of the bilinear kernel) and the 2 -> 141 nearest-exact tie.
    Largest d of the float32 restatement seen per mode on these shapes: bilinear 1.1e-7, bicubic 2.4e-7, area 2.0e-7 (the kernels
    gave the restatement's own bits: they are compiled without FMA contraction)."""
    _check_resize(native, dev, mode, ac, RC.PLANES, shape[0], shape[1], 31)


@pytest.mark.parametrize("mode,ac", RC.MODE_CASES, ids=RC.MODE_IDS)
def test_single_resize_second_grid_pass(mode, ac, dev, native):
    """Just past one grid pass (256 * 32 workgroups of 256 threads): the tail of the outputs is produced by the second trip of the
    grid-stride loop, forward and backward.  Largest d seen: bilinear 1.3e-7, bicubic 2.7e-7, area 7.5e-8."""
    planes, src, size = RC.grid_stride_case(mode)
    _check_resize(native, dev, mode, ac, planes, src, size, 32)


# ------------------------------------------------------------------------------------------------- direct C ABI calls
def _c_flip(N, dev, maps, views, inner, outer, size, ac):
    """ptb_ms_flip_deaug_reduce itself: (return code, output tensor pre-filled with NaN)."""
    lib = N.load()
    V = len(views)
    B, C = maps[0].shape[0] // V, maps[0].shape[1]
    out = torch.full((B, C) + tuple(size), float("nan"), device=dev, dtype=torch.float32)
    hs, ws = N.int_array([int(m.shape[2]) for m in maps]), N.int_array([int(m.shape[3]) for m in maps])
    ptrs = _resample()._ptr_array(maps)
    with N.on_device(dev):
        rc = lib.ptb_ms_flip_deaug_reduce(ptrs, hs, ws, len(maps), V, N.int_array(list(views)), inner, out.data_ptr(), B * C, size[0], size[1],
                                          1 if ac else 0, outer, N.stream_ptr(dev))
    return rc, out


def _c_ms(N, dev, maps, outer, size, ac):
    """ptb_ms_deaug_reduce itself (the tiled or the plain kernel, by tunable 3)."""
    lib = N.load()
    B, C = maps[0].shape[0], maps[0].shape[1]
    out = torch.full((B, C) + tuple(size), float("nan"), device=dev, dtype=torch.float32)
    hs, ws = N.int_array([int(m.shape[2]) for m in maps]), N.int_array([int(m.shape[3]) for m in maps])
    ptrs = _resample()._ptr_array(maps)
    with N.on_device(dev):
        rc = lib.ptb_ms_deaug_reduce(ptrs, hs, ws, len(maps), out.data_ptr(), B * C, size[0], size[1], 1 if ac else 0, outer, N.stream_ptr(dev))
    return rc, out


D_SEEN = {"d": 0.0, "kernel": 0.0}      # largest deviation of the float32 restatement / of a kernel in the linear merges so far (printed)


def _assert_merge(got, ref, d, what):
    """d is None: non-linear reduction (rtol = atol = 1e-5); else the linear bound 4 d + 1e-7."""
    if d is None:
        assert _close(got, ref, 1e-5, 1e-5), (what, _worst(got, ref))
    else:
        D_SEEN["d"], D_SEEN["kernel"] = max(D_SEEN["d"], d), max(D_SEEN["kernel"], _worst(got, ref))
        assert _worst(got, ref) <= 4 * d + 1e-7, (what, _worst(got, ref), d)


# ------------------------------------------------------------------------------------------------- B. multiscale merge, three kernels
MS_PATHS = {"fused": {}, "tiled": dict(k1=1), "plain": dict(k1=1, k3=0)}
SEEN_FUSED = {}


@pytest.mark.parametrize("set_name", list(RC.ms_source_sets((72, 136))))
@pytest.mark.parametrize("size", RC.MS_OUT_SIZES, ids=lambda s: "%dx%d" % s)
def test_ms_merge_three_kernels(size, set_name, dev, native):
    """tta.ms_image_deaugment and the C ABI on output widths with wout % 4 = 0, 3, 1, 2, each through ptb_ms_flip_deaug_reduce with one
    view (default), ms_reduce_tiled_kernel (tunable 1 = 1) and ms_reduce_kernel (tunables 1 = 1, 3 = 0).  The sets reach the un-staged
    branch of the tiled kernel next to staged scales (ratios 0.5 and 3 in one launch; 1.5 along one axis only), one and eight scales, and
    source widths that are no multiple of 4.  mean and gmean everywhere, all seven reductions on the ratio {0.5, 1, 3} set.
    Largest d of the float32 restatement seen for the linear merges: 3.3e-7 (the sum of eight scales); the kernels came as close."""
    N = native
    lib = N.load()
    tta = _tta()
    sources = RC.ms_source_sets(size)[set_name]
    maps = [RC.uniform(RC.PLANES + s, 40 + i) for i, s in enumerate(sources)]
    t64 = [torch.from_numpy(m.astype(np.float64)) for m in maps]
    gpu = [torch.from_numpy(m).to(dev) for m in maps]
    offs = RC.offsets_for(sources, size)
    reductions = RO.REDUCTIONS if set_name == "half_one_three" else ("mean", "gmean")
    for ac in (False, True):
        for red in reductions:
            code = RO.REDUCTIONS.index(red)
            ref = RO.ms_merge_t(t64, size, red, ac).numpy()
            d = _worst(AO.ms_image_deaugment(maps, offs, red, ac), ref) if red in RO.LINEAR_REDUCTIONS else None
            for path, keys in MS_PATHS.items():
                with tunables(lib, **keys):
                    rc, direct = _c_flip(N, dev, gpu, VIEWS["ident"], N.RED_SUM, code, size, ac)
                    if path != "fused":
                        assert rc == N.PTB_EUNSUPPORTED       # forced off: the merge kernels proper are what runs below
                    if rc != 0:
                        assert rc == N.PTB_EUNSUPPORTED
                        rc2, direct = _c_ms(N, dev, gpu, code, size, ac)
                        assert rc2 == 0
                    else:
                        SEEN_FUSED[(size, set_name)] = True
                    before = N.calls
                    out = tta.ms_image_deaugment(gpu, offs, reduction=red, align_corners=ac)
                    assert N.calls == before + 1
                what = (size, set_name, red, ac, path, rc)
                _assert_merge(direct.cpu().numpy(), ref, d, what)
                assert torch.equal(out, direct), what
    print("linear merges so far:", D_SEEN)
    if size[1] % 4 == 0 and set_name in ("one_same", "one_resized", "mild_mult4"):
        assert SEEN_FUSED.get((size, set_name)), "the fused kernel never took a shape well inside its windows"
    if size[1] % 4 or set_name in ("half_one_three", "odd_widths"):
        assert not SEEN_FUSED.get((size, set_name)), "ratio 3 / widths that are no multiple of 4 are not for the fused kernel"


# ------------------------------------------------------------------------------------------------- C. acceptance boundary
C_OUT = (72, 136)
C_HEIGHTS = [(h, 136) for h in range(86, 117)]
C_WIDTHS = [(72, w) for w in range(160, 221, 4)]
INNERS, OUTERS = ("mean", "gmean", "hmean"), ("mean", "gmean", "sum")
_C_REFS = {}


def _c_case(group, src, ac):
    """Inputs and float64 references of one walked source size (shared by the six tile shapes): maps = [walked scale, output-size scale],
    {(inner, outer): (ref, d or None)}."""
    key = (group, src, ac)
    if key not in _C_REFS:
        V = len(VIEWS[group])
        sources = [src, C_OUT]
        maps = [RC.uniform((V * 1, 2) + s, 50 + i + 7 * src[0] + src[1]) for i, s in enumerate(sources)]
        t64 = [torch.from_numpy(m.astype(np.float64)) for m in maps]
        offs = RC.offsets_for(sources, C_OUT)
        refs = {}
        for inner in (INNERS if V > 1 else ("mean",)):
            per_scale = [AO.image_deaugment(m, group, inner) for m in maps] if V > 1 else maps
            for outer in OUTERS:
                ref = RO.ms_merge_t(t64, C_OUT, outer, ac, views=VIEWS[group], inner=inner).numpy()
                linear = inner == "mean" and outer in RO.LINEAR_REDUCTIONS
                refs[(inner, outer)] = (ref, _worst(AO.ms_image_deaugment(per_scale, offs, outer, ac), ref) if linear else None)
        _C_REFS[key] = (maps, offs, refs)
    return _C_REFS[key]


def _python_entry(tta, group, gpu, offs, inner, outer, ac):
    if group == "ident":
        return tta.ms_image_deaugment(gpu, offs, reduction=outer, align_corners=ac)
    return tta.ms_flips_image_deaugment(gpu, offs, group=group, inner_reduction=inner, reduction=outer, align_corners=ac)


def _walk(N, dev, group, sizes, ac):
    """Every source size of one walk: accepted calls match the model, refused ones return PTB_EUNSUPPORTED and the Python entry still
    gives the right values.  Returns {size: accepted}."""
    tta = _tta()
    seen = {}
    for src in sizes:
        maps, offs, refs = _c_case(group, src, ac)
        gpu = [torch.from_numpy(m).to(dev) for m in maps]
        for (inner, outer), (ref, d) in refs.items():
            rc, out = _c_flip(N, dev, gpu, VIEWS[group], RO.REDUCTIONS.index(inner), RO.REDUCTIONS.index(outer), C_OUT, ac)
            what = (group, src, ac, inner, outer, rc)
            assert seen.setdefault(src, rc == 0) == (rc == 0), what           # acceptance is a matter of geometry, not of the reduction
            if rc == 0:
                _assert_merge(out.cpu().numpy(), ref, d, what)
            else:
                assert rc == N.PTB_EUNSUPPORTED, what
                _assert_merge(_python_entry(tta, group, gpu, offs, inner, outer, ac).cpu().numpy(), ref, d, what)
    return seen


@pytest.mark.parametrize("group", list(VIEWS))
@pytest.mark.parametrize("tile_rows", [16, 32, 64])
@pytest.mark.parametrize("tile_w", [64, 128])
def test_fused_acceptance_boundary(tile_w, tile_rows, group, dev, native):
    """ptb_ms_flip_deaug_reduce with 1, 2 (fliplr; flipud) and 4 (d2) views on a (72, 136) output, both align_corners, per tile shape
    (tunable 15 x tunable 6): the source height walks 86 .. 116 at width 136, the source width 160 .. 220 in steps of 4 at height 72 --
    through the host rule (need_r, need_c, wide_ok) that decides whether a tile's source window fits the LDS window the device clamps
    to.  Each walk must see accepted and refused sizes, accepted below refused, and every answer must be right: a bound that is off
    by one gives wrong pixels, not a fault.
    Last accepted sizes seen: height 99 (align_corners=False) and 98 (True) / 96 / 95 for 16 / 32 / 64-row tiles, width 188 whatever
    tunable 15 says: at 128 the launch falls back to the 64-wide tiles where the wide windows no longer fit, so the sizes on either side
    of that inner line are all accepted and all checked."""
    N = native
    lib = N.load()
    assert _tta().DEAUGMENT_VIEWS.get(group, (0,)) == VIEWS[group]
    with tunables(lib, k15=tile_w, k6=tile_rows):
        for ac in (False, True):
            for axis, sizes in (("height", C_HEIGHTS), ("width", C_WIDTHS)):
                seen = _walk(N, dev, group, sizes, ac)
                accepted = [s for s in sizes if seen[s]]
                refused = [s for s in sizes if not seen[s]]
                print(f"tile {tile_w} x {tile_rows}, {group}, align_corners={ac}, {axis}: last accepted {accepted[-1:]}, first refused {refused[:1]}")
                print("linear merges so far:", D_SEEN)
                assert accepted and refused, (axis, ac)
                assert max(accepted) < min(refused), (axis, ac)


# LDS window rows of ms_flip_reduce_kernel per tile height (FZ_LR16 / FZ_LR32 / FZ_LR)
FULL_WINDOW_ROWS = {16: 25, 32: 46, 64: 88}


@pytest.mark.parametrize("group", ["ident", "flipud"])
@pytest.mark.parametrize("tile_rows", [16, 32, 64])
def test_fused_full_lds_window(tile_rows, group, dev, native):
    """A source map of exactly as many rows as the LDS window holds, under a single output tile that reads all of them (a window
    never exceeds the map, so the host rule takes the map whatever the ratio): every window row is filled and read.  One row more
    is refused.  The window extent is computed here from the taps, not assumed."""
    N = native
    lib = N.load()
    rows = FULL_WINDOW_ROWS[tile_rows]
    size = (tile_rows - 3, 72)
    with tunables(lib, k15=64, k6=tile_rows):
        for ac in (False, True):
            for h, expect in ((rows, True), (rows + 1, False)):
                src = (h, 92)
                assert RC.window_extent(h, size[0], ac, tile_rows) == h                   # the one tile's taps span the whole map
                V = len(VIEWS[group])
                maps = [RC.uniform((V, 2) + src, 60 + h), RC.uniform((V, 2) + size, 61 + h)]
                t64 = [torch.from_numpy(m.astype(np.float64)) for m in maps]
                gpu = [torch.from_numpy(m).to(dev) for m in maps]
                for inner, outer in (("mean", "mean"), ("gmean", "gmean")):
                    ref = RO.ms_merge_t(t64, size, outer, ac, views=VIEWS[group], inner=inner).numpy()
                    per_scale = [AO.image_deaugment(m, group, inner) for m in maps] if V > 1 else maps
                    d = _worst(AO.ms_image_deaugment(per_scale, RC.offsets_for([src, size], size), outer, ac), ref) if inner == "mean" else None
                    rc, out = _c_flip(N, dev, gpu, VIEWS[group], RO.REDUCTIONS.index(inner), RO.REDUCTIONS.index(outer), size, ac)
                    what = (tile_rows, group, ac, src, inner, rc)
                    assert (rc == 0) == expect and rc in (0, N.PTB_EUNSUPPORTED), what
                    if rc == 0:
                        _assert_merge(out.cpu().numpy(), ref, d, what)
                    else:
                        _assert_merge(_python_entry(_tta(), group, gpu, RC.offsets_for([src, size], size), inner, outer, ac).cpu().numpy(), ref, d, what)


# ------------------------------------------------------------------------------------------------- D. backward of the merge
@pytest.mark.parametrize("reduction", RO.REDUCTIONS)
def test_ms_merge_backward(reduction, dev, native):
    """ms_image_deaugment(...).backward() (ms_reduce_bwd_kernel) on a (36, 52) output from (12, 20), (36, 52), (108, 156) -- ratios 1 / 3
    and 3, many output pixels per source pixel and the reverse -- against autograd of the float64 model."""
    tta = _tta()
    size = (36, 52)
    sources = [(12, 20), (36, 52), (108, 156)]
    maps = [RC.uniform(RC.PLANES + s, 70 + i) for i, s in enumerate(sources)]
    offs = RC.offsets_for(sources, size)
    for ac in (False, True):
        t64 = [torch.from_numpy(m.astype(np.float64)).requires_grad_(True) for m in maps]
        ref = RO.ms_merge_t(t64, size, reduction, ac)
        g = RC.grad_weights(tuple(ref.shape))
        (ref * torch.from_numpy(g.astype(np.float64))).sum().backward()
        gpu = [torch.from_numpy(m).to(dev).requires_grad_(True) for m in maps]
        before = native.calls
        out = tta.ms_image_deaugment(gpu, offs, reduction=reduction, align_corners=ac)
        (out * torch.from_numpy(g).to(dev)).sum().backward()
        assert native.calls == before + 2
        if reduction in RO.LINEAR_REDUCTIONS:
            d = _worst(AO.ms_image_deaugment(maps, offs, reduction, ac), ref.detach().numpy())
            _assert_merge(out.detach().cpu().numpy(), ref.detach().numpy(), d, (reduction, ac))
        else:
            _assert_merge(out.detach().cpu().numpy(), ref.detach().numpy(), None, (reduction, ac))
        for t, r in zip(gpu, t64):
            np.testing.assert_allclose(t.grad.cpu().numpy(), r.grad.numpy(), rtol=2e-4, atol=2e-5)


# ------------------------------------------------------------------------------------------------- E. nearest-exact ties
def test_nearest_exact_ties_follow_device_aten(dev, native):
    """torch.nn.functional.interpolate(mode='nearest-exact') on the DEVICE -- what the unmodified reference runs there -- at every pair
    n_in, n_out <= 300 where the float32 rule floorf((dst + 0.5f) * scale) and the exact rational rule select different pixels (1 845
    pairs, among them the 32 where CPU ATen leaves the float32 rule: 2 -> 141, 2 -> 159, 2 -> 165, 4 -> 166, ...).

    Observed on an MI355X (torch 2.10, ROCm 7.0): device ATen selects the pixels of the float32 rule on all of them, along either axis --
    the same pixels as resize_nearest_exact_kernel and the model.  The kernel stays as it is; the CPU is the odd one out at the ties."""
    ties = RC.nearest_exact_tie_pairs(300)
    assert {(2, 141), (2, 159), (2, 165), (4, 166)} <= set(ties)
    resize = _resample().resize
    rows = {n: torch.arange(n, dtype=torch.float32, device=dev).reshape(1, 1, n, 1) for n in {p[0] for p in ties}}
    bad_kernel, bad_aten = [], []
    for (n_in, n_out), positions in ties.items():
        x = rows[n_in]
        aten = F.interpolate(x, size=(n_out, 1), mode="nearest-exact").flatten()
        aten_w = F.interpolate(x.reshape(1, 1, 1, n_in), size=(1, n_out), mode="nearest-exact").flatten()
        ours = resize(x, (n_out, 1), "nearest-exact", None).flatten()
        ours_w = resize(x.reshape(1, 1, 1, n_in), (1, n_out), "nearest-exact", None).flatten()
        model = torch.from_numpy(RO.nearest_index(n_in, n_out, True).astype(np.float32)).to(dev)
        if not (torch.equal(ours, model) and torch.equal(ours_w, model)):
            bad_kernel.append((n_in, n_out))
        if not (torch.equal(aten, ours) and torch.equal(aten_w, ours)):
            bad_aten.append((n_in, n_out))
    assert not bad_kernel, bad_kernel[:8]
    assert not bad_aten, bad_aten[:8]
