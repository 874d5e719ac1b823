"""GPU: the deferred band merge of fp16 / bf16 d4 model outputs on pairs of work items (csrc/ptb_bandpair.hip) computes, bit for bit,
what the incremental merger computes (``TileMerger(auto_plan=False)`` + ``merge()``) and what the same deferred merger computes one
64 x 64 item per workgroup (``ptb_set_tunable(28, 0)``).  The geometries are the smallest that reach each branch of the dispatch: a
3 x 3 grid of tiles gives items under 1, 2 and 4 covering tiles; the band height decides whether a launch group is pairs only, pairs
plus 64-row or 32-row singles, or has no pair at all (``ptb_band_plan_pairs`` says which, and the test checks that it is the one meant)."""
import ctypes

import pytest
import torch

from oracle import tiles_oracle as TO

pytestmark = pytest.mark.gpu

C = 3
DTYPES = [torch.float16, torch.bfloat16]
#                 image, tile, step, what its launch groups must hold
GEOMETRIES = {
    "pairs only": ((512, 512), 256, 128, "pairs"),                 # bands of 128 rows
    "pair + 64-row single": ((768, 768), 384, 192, "both"),         # bands of 192 rows: two launches per group
    "pair + 32-row single": ((640, 640), 320, 160, "both"),         # bands of 160 rows; cells 160 wide: items of 64, 64 and 32 columns
    "one item row per band": ((256, 256), 128, 64, "singles"),      # nothing to pair, and no empty launch
    "rows off the 8-pixel grid": ((520, 520), 256, 132, "singles"),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(merger, outputs, crops, batch, literal, reduction):
    from pytorch_toolbelt_amd.inference import tta

    n = len(crops)
    for b0 in range(0, n, batch):
        b1 = min(n, b0 + batch)
        y = torch.cat([outputs[k * n + b0:k * n + b1] for k in range(8)])       # chunk-major model output of the batch
        if literal:
            merger.integrate_batch(tta.d4_image_deaugment(y, reduction=reduction), crops[b0:b1])
        else:
            merger.integrate_batch_deaugment(y, crops[b0:b1], group="d4", reduction=reduction)
    return merger.merge()


def _layout(merger):
    """[(pair_cnt, single_cnt)] of the launch groups of a deferred merger's band plan."""
    from pytorch_toolbelt_amd import _native as N

    lib, handle = N.load(), merger._bands.handle
    ng = ctypes.c_int()
    assert lib.ptb_band_plan_info(handle, ctypes.byref(ng), None, None, None, None) == 0
    out = []
    for g in range(ng.value):
        pc, sc = ctypes.c_int(), ctypes.c_int()
        assert lib.ptb_band_plan_pairs(handle, g, ctypes.byref(pc), ctypes.byref(sc)) == 0
        out.append((pc.value, sc.value))
    return out


def _same(a, b):
    """torch.equal, a NaN (uncovered pixels: 0 / 0 like the reference's merge) counting as equal to a NaN in the same place."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def _check(dev, name, dtype, batch=8, literal=False, reduction="mean", defer_rows=None, extra_rows=0, seed=5):
    from pytorch_toolbelt_amd import _native as N
    from pytorch_toolbelt_amd.inference.tiles import TileMerger

    shape, tile, step, holds = GEOMETRIES[name]
    geom = TO.slicer_geometry(shape, tile, step)
    crops = geom["crops"]
    target = (geom["target_shape"][0] + extra_rows, geom["target_shape"][1])
    w = TO.pyramid_window(tile, tile)[0]
    n = len(crops)
    g = torch.Generator(device=dev).manual_seed(seed)
    outputs = (torch.rand((8 * n, C, tile, tile), device=dev, generator=g) * 0.9 + 0.05).to(dtype)
    want = _run(TileMerger(target, C, w, device=dev, auto_plan=False), outputs, crops, batch, literal, reduction)

    def deferred():
        m = TileMerger(target, C, w, device=dev, crops=crops, defer=True, defer_rows=defer_rows)
        out = _run(m, outputs, crops, batch, literal, reduction)
        assert m._bands is not None and m._bands_done == len(m._bands.bands), "the deferred band merge did not run"
        return m, out

    m, got = deferred()
    layout = _layout(m)
    pairs, singles = sum(p for p, _ in layout), sum(s for _, s in layout)
    assert {"pairs": pairs > 0 and (singles == 0 or extra_rows > 0), "both": pairs > 0 and singles > 0, "singles": pairs == 0 and singles > 0}[holds], layout
    lib = N.load()
    assert lib.ptb_set_tunable(28, 0) == 0
    try:
        _, unpaired = deferred()
    finally:
        assert lib.ptb_set_tunable(28, 1) == 0
    if extra_rows:
        assert torch.isnan(want[:, -extra_rows:]).all() and not torch.isnan(want[:, :-extra_rows]).any()
        assert _same(got, want) and _same(got, unpaired)
    else:
        assert torch.equal(got, want), "paired items differ from the incremental merge"
        assert torch.equal(got, unpaired), "paired items differ from one item per workgroup"
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_every_branch_of_the_dispatch(name, dtype, dev):
    """Batches of 8 with a ragged last one (9 tiles)."""
    _check(dev, name, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", ["pairs only", "pair + 32-row single"])
def test_gmean(name, dtype, dev):
    _check(dev, name, dtype, reduction="gmean", seed=6)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", ["pairs only", "pair + 64-row single"])
def test_literal_calls_round_to_the_source_type(name, dtype, dev):
    """integrate_batch(tta.d4_image_deaugment(y), crops): the reduced value is rounded to y's dtype before it is blended."""
    _check(dev, name, dtype, literal=True, seed=7)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_batches_of_one(dtype, dev):
    _check(dev, "pair + 32-row single", dtype, batch=1, seed=8)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_launch_groups_of_256_rows_give_the_default_groups_bits(dtype, dev):
    a = _check(dev, "pair + 64-row single", dtype, defer_rows=256, seed=9)
    b = _check(dev, "pair + 64-row single", dtype, seed=9)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_uncovered_rows_merge_to_nan(dtype, dev):
    """64 rows below the last tile row: a band without tiles rides with its neighbour's launch, its items are singles and 0 / 0."""
    _check(dev, "pairs only", dtype, extra_rows=64, seed=10)
