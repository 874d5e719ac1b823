"""GPU: the deferred band launches sum the normaliser themselves, from the window values they blend with, and do not read the plan's
normaliser map.  Every case hands the deferred merger a map full of NaN -- a single read of it would show in the result -- and
asks for the incremental merger's bits (``auto_plan=False``: accumulate, then divide by the accumulated normaliser), NaN positions
and NaN payloads included: the maps are compared as int32.  Tiles are 64 x 64 throughout; the images are a few hundred pixels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
TILE = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _slicer(shape, step, tile=TILE):
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer

    return ImageSlicer(tuple(shape) + (3,), tile, step, weight="pyramid")


def _batches(crops, C, n_views, dtype, bs, seed):
    """[(chunk-major [V * nb, C, 64, 64] batch on the host, its crops)] for the whole crop list."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for b0 in range(0, len(crops), bs):
        c = np.ascontiguousarray(crops[b0:b0 + bs], dtype=np.int64)
        out.append((torch.randn((n_views * len(c), C, TILE, TILE), generator=g).to(dtype), c))
    return out


def _feed(m, fed, dev, group, reduction="mean", activation=None, layout=None):
    for y, crops in fed:
        y = y.to(dev)
        if layout is not None:
            y = y.contiguous(memory_format=layout)
        kw = dict(activation=activation, temperature=0.75) if activation is not None else {}
        if group is None:
            m.integrate_batch(y, crops, **kw)
        else:
            m.integrate_batch_deaugment(y, crops, group=group, reduction=reduction, **kw)


def _same_bits(got, want, what):
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape, what
    a, b = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} values differ in their bits"


def _poisoned_equals_incremental(dev, target_shape, weight, crops, C, fed, group, what, defer_rows=None, **feed_kw):
    """The deferred merger with a NaN normaliser map against the incremental one; returns the merged map."""
    from pytorch_toolbelt_amd.inference.tiles import TileMerger

    inc = TileMerger(target_shape, C, weight, device=dev, auto_plan=False)
    _feed(inc, fed, dev, group, **feed_kw)
    assert inc.mode == "incremental"
    want = inc.merge()
    d = TileMerger(target_shape, C, weight, device=dev, crops=crops, defer=True, defer_rows=defer_rows)
    assert d._bands is not None, f"{what}: the band plan did not take this geometry"
    d._plan.norm_full.fill_(float("nan"))
    _feed(d, fed, dev, group, **feed_kw)
    assert d.mode == "deferred bands" and d._bands_done == len(d._bands.bands) and not d._held, what
    got = d.merge()
    _same_bits(got, want, what)
    return got


# ------------------------------------------------------------------------------------------------ poisoned normaliser: every kernel path
N_VIEWS = dict(d4=8, fliplr=2)


@pytest.mark.parametrize("group,dtype,C", [
    ("d4", torch.float32, 3),          # prefetch + LDS
    ("d4", torch.bfloat16, 3),
    (None, torch.float32, 1),          # identity view: the channel loop
    (None, torch.float32, 3),
    (None, torch.float16, 1),
    (None, torch.float16, 3),
    ("fliplr", torch.float32, 2),      # every covering tile requested up front, one workgroup per channel
], ids=lambda v: str(v).split(".")[-1])
def test_poisoned_normaliser(group, dtype, C, dev):
    s = _slicer((200, 264), 32)
    fed = _batches(s.crops, C, N_VIEWS.get(group, 1), dtype, 5, 1)
    _poisoned_equals_incremental(dev, s.target_shape, s.weight, s.crops, C, fed, group, f"{group} {dtype} C={C}")


def test_poisoned_normaliser_plain_loop(dev):
    """The instances without prefetch: all of them with the prefetch switched off (ptb_set_tunable key 21), and the one that reads its
    view codes at run time, for a view set that is none of the compiled groups (the public calls name a group, so the set is entered
    into the group table for the length of the test)."""
    from pytorch_toolbelt_amd import _native as N
    from pytorch_toolbelt_amd.inference import tta

    s = _slicer((200, 264), 32)
    lib = N.load()
    assert lib.ptb_set_tunable(21, 0) == 0
    try:
        for group, dtype in (("d4", torch.float32), ("d4", torch.bfloat16), (None, torch.float32)):
            fed = _batches(s.crops, 3, N_VIEWS.get(group, 1), dtype, 5, 2)
            _poisoned_equals_incremental(dev, s.target_shape, s.weight, s.crops, 3, fed, group, f"no prefetch {group} {dtype}")
    finally:
        assert lib.ptb_set_tunable(21, 2) == 0
    name = "band-norm-test-rot180-transpose"
    assert name not in tta.DEAUGMENT_VIEWS
    tta.DEAUGMENT_VIEWS[name] = (N.IDENT, N.ROT180, N.TRANSPOSE)
    try:
        fed = _batches(s.crops, 2, 3, torch.float32, 5, 3)
        _poisoned_equals_incremental(dev, s.target_shape, s.weight, s.crops, 2, fed, name, "run-time view codes")
    finally:
        del tta.DEAUGMENT_VIEWS[name]


@pytest.mark.parametrize("layout", [None, CL], ids=["planar", "channels_last"])
@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
def test_poisoned_normaliser_activation(activation, layout, dev):
    """tact_plan_kernel (planar) and tact_cl_plan_kernel (channels_last)."""
    s = _slicer((200, 264), 32)
    for group, dtype, C in (("d4", torch.float32, 3), (None, torch.bfloat16, 5)):
        fed = _batches(s.crops, C, N_VIEWS.get(group, 1), dtype, 5, 4)
        _poisoned_equals_incremental(dev, s.target_shape, s.weight, s.crops, C, fed, group, f"{activation} {layout} {group}", activation=activation,
                                     layout=layout)


def test_poisoned_normaliser_channels_last(dev):
    """cl_plan_kernel: channels_last model outputs without an activation."""
    s = _slicer((200, 264), 32)
    for group, dtype, C in (("d4", torch.float32, 3), (None, torch.float16, 6), ("fliplr", torch.bfloat16, 4)):
        fed = _batches(s.crops, C, N_VIEWS.get(group, 1), dtype, 5, 5)
        _poisoned_equals_incremental(dev, s.target_shape, s.weight, s.crops, C, fed, group, f"channels_last {group} {dtype}", layout=CL)


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("defer_rows", [64, 1 << 20])
@pytest.mark.parametrize("step,covers", [(32, {1, 2, 4}), ((64, 24), {1, 2, 3})], ids=["step32", "step64x24"])
def test_geometry_ragged_items(step, covers, defer_rows, dev):
    """A 100 x 150 image: work items ragged in both axes; one, two and four (step 32) or up to three (step (64, 24)) tiles over a pixel."""
    s = _slicer((100, 150), step)
    H, W = s.target_shape
    cover = np.zeros((H, W), dtype=int)
    for x, y, w, h in s.crops:
        cover[y:y + h, x:x + w] += 1
    assert set(np.unique(cover)) == covers, np.unique(cover)
    for group, C in (("d4", 3), (None, 2)) if step == 32 else ((None, 2), ("fliplr", 3)):
        fed = _batches(s.crops, C, N_VIEWS.get(group, 1), torch.float32, 4, 6)
        got = _poisoned_equals_incremental(dev, s.target_shape, s.weight, s.crops, C, fed, group, f"step {step} {group}", defer_rows=defer_rows)
        assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("defer_rows", [64, 1 << 20])
def test_uncovered_column_stays_nan(defer_rows, dev):
    """An explicit crop list that leaves columns 128:192 without a tile: 0 / 0 there, with the bits the incremental merge gives it."""
    w = _slicer((128, 128), 32).weight
    crops = np.array([[x, y, TILE, TILE] for y in (0, 32, 64) for x in (0, 32, 64, 192)], dtype=np.int64)
    H, W = 128, 256
    for group, C, kw in (("d4", 2, {}), (None, 3, {}), (None, 3, dict(layout=CL)), ("d4", 2, dict(activation="sigmoid"))):
        fed = _batches(crops, C, N_VIEWS.get(group, 1), torch.float32, 5, 7)
        got = _poisoned_equals_incremental(dev, (H, W), w, crops, C, fed, group, f"hole {group} {kw}", defer_rows=defer_rows, **kw)
        nan = torch.isnan(got)
        assert bool(nan[:, :, 128:192].all()) and not bool(nan[:, :, :128].any()) and not bool(nan[:, :, 192:].any())


def test_window_with_a_row_of_zeros(dev):
    """Window values that are exactly zero: where only such values cover a pixel the sum and the normaliser are both zero -- the NaN / inf
    pattern is the incremental merge's."""
    s = _slicer((100, 150), 64)                # no overlap: the zero row of every tile is 0 / 0
    w = np.array(s.weight, dtype=np.float32, copy=True)
    w[10, :] = 0
    w[:, 7] = 0
    overlapping = _slicer((100, 150), 32)
    for sl in (s, overlapping):
        for group, C in (("d4", 2), (None, 3)):
            fed = _batches(sl.crops, C, N_VIEWS.get(group, 1), torch.float32, 4, 8)
            got = _poisoned_equals_incremental(dev, sl.target_shape, w, sl.crops, C, fed, group, f"zero row {group}")
            assert bool(torch.isnan(got).any())


# ------------------------------------------------------------------------------------------------ sharded: partial rows keep undivided sums
class _Rank:
    """Rank / world stand-in: the ranks are played one after the other and their rectangles are handed over by hand."""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world

    def get_rank(self, group=None):
        return self.rank

    def get_world_size(self, group=None):
        return self.world


def test_sharded_partial_rows_carry_undivided_sums(dev):
    """world = 3, partition="tiles", defer=True.  The rows a rank shares with a neighbour leave its launches as undivided sums (the
    rectangles it hands over are the accumulator of an incremental merger fed the rank's tiles, bit for bit; the neighbours' sums are
    added and the total divided afterwards), and the assembled map is the single-device merge.  A rank issues the tiles its neighbours
    wait for first, so the rows it finishes alone sum in ITS order and are divided by the normaliser map it is handed -- summed in the
    image's order: ``ptb_band_plan_submit_rank`` keeps reading the map, and those rows are (the rank's sums) / (the image's map), bit for bit."""
    from pytorch_toolbelt_amd.inference.tiles import TileMerger
    from pytorch_toolbelt_amd.parallel import ShardedTileMerger

    s = _slicer((420, 200), 32)
    crops, C, world = np.ascontiguousarray(s.crops, dtype=np.int64), 2, 3
    g = torch.Generator().manual_seed(9)
    views = torch.randn((len(crops), 8, C, TILE, TILE), generator=g).to(dev)

    def batch(idx):
        return views[idx].transpose(0, 1).reshape(-1, C, TILE, TILE).contiguous()

    def incremental(tiles):
        m = TileMerger(s.target_shape, C, s.weight, device=dev, auto_plan=False)
        for b0 in range(0, len(tiles), 4):
            m.integrate_batch_deaugment(batch(tiles[b0:b0 + 4]), crops[tiles[b0:b0 + 4]], group="d4")
        return m

    ref = incremental(np.arange(len(crops)))
    norm = ref.norm_mask.clone()
    want = ref.merge()
    ranks, sums = [], []
    for r in range(world):
        m = ShardedTileMerger(s.target_shape, C, s.weight, crops, device=dev, dist=_Rank(r, world), partition="tiles", defer=True)
        assert m._deferred is not None and m._deferred.final[1] > m._deferred.final[0], "the case needs rows every rank finishes alone"
        m._start_exchange = lambda m=m: setattr(m, "_exchanged", True)
        for b0 in range(0, len(m.tiles), 4):
            idx = m.tiles[b0:b0 + 4]
            m.integrate_batch_deaugment(batch(idx), crops[idx], group="d4")
        ranks.append(m)
        sums.append(incremental(np.asarray(m.tiles)).image.clone())       # the rank's weighted sums, in the rank's order
    assert any(np.any(np.diff(np.asarray(m.tiles)) < 0) for m in ranks), "the case needs a rank that issues its boundary tiles first"
    shared_rows = 0
    for m in ranks:
        for buf, (src, r0, r1, c0, c1) in zip(m._recv_buf, m.recvs):
            rect = ranks[src]._rect(r0, r1, c0, c1)
            _same_bits(rect.contiguous(), sums[src][:, r0:r1, c0:c1].contiguous(), f"partial sums of rank {src}, rows {r0}:{r1}")
            buf.copy_(rect)
            shared_rows += r1 - r0
    assert shared_rows > 0
    full = torch.full_like(want, float("nan"))
    for r, m in enumerate(ranks):
        o0, o1 = m.owned_rows
        full[:, o0:o1] = m.merge()
        f0, f1 = m._deferred.final
        quotient = (sums[r][:, f0:f1].double() / norm[:, f0:f1].double()).float()      # (__fdiv_rn's value: the float64 quotient rounded once more)
        _same_bits(full[:, f0:f1], quotient, f"rows {f0}:{f1} that rank {r} finishes alone")
    assert bool(torch.isfinite(full).all())
    # (a shared row adds its own rank's tiles first, then the neighbour's partial sum: another order of fp32 additions)
    assert float((full - want).abs().max()) <= 1e-5
