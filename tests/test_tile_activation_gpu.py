"""``activation=`` / ``temperature=`` of the 2-D de-augmentations and the tile mergers on the GPU (csrc/ptb_tile_activation.hip): every fused
call against the float64 model of tests/tile_activation_cases.py (1e-5 absolute), and bit identity between the library's own paths --
dense and channels-last sources, the incremental and the deferred merger, the fused merge and de-augment-then-merge.  On the parent
commit every test here raises TypeError on the keyword."""
import warnings

import pytest
import torch

import tile_activation_cases as K

pytestmark = pytest.mark.gpu

CL = torch.channels_last
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
N_VIEWS = {None: 1, "fliplr": 2, "flipud": 2, "flips": 3, "d2": 4, "d4": 8}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _slicer(shape, tile, step):
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer

    return ImageSlicer(tuple(shape) + (3,), tile, step, weight="pyramid")


def _merger(slicer, C, dev, **kw):
    from pytorch_toolbelt_amd.inference.tiles import TileMerger

    return TileMerger(slicer.target_shape, C, slicer.weight, device=dev, **kw)


def _channels(activation):
    return (1, 3, 4, 5, 16) + ((19,) if activation == "sigmoid" else ())


# ------------------------------------------------------------------------------------------------ reduce
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("activation", K.ACTIVATIONS)
@pytest.mark.parametrize("group", K.GROUPS)
def test_deaugment(group, activation, dtype, dev):
    from pytorch_toolbelt_amd import _native as N
    from pytorch_toolbelt_amd.inference import tta

    fn = getattr(tta, f"{group}_image_deaugment")
    V = N_VIEWS[group]
    # 64 / 128: one and several chunks of the vector kernels; 100: the last chunk is ragged; 102: off the 4-pixel grid (torch-op fallback for
    # planar sources); 52 x 36: non-square, the non-transposing groups
    sizes = [(64, 64), (128, 128), (100, 100), (102, 102)] + ([(52, 36)] if group != "d4" else [])
    for C in _channels(activation):
        for k, (H, W) in enumerate(sizes):
            red = K.REDUCTIONS[(C + k) % 3]
            y = K.logits((V * 2, C, H, W), dtype, 100 * C + k)
            want = K.deaugment64(y, group, red, activation, 0.7)
            yd = y.to(dev)
            calls = N.calls
            got = fn(yd, reduction=red, activation=activation, temperature=0.7)
            assert type(got) is torch.Tensor and got.dtype == torch.float32 and got.is_contiguous() and N.calls > calls
            K.assert_close(got, want, f"{group} {activation} C={C} {H}x{W} {red}")
            got_cl = fn(yd.contiguous(memory_format=CL), reduction=red, activation=activation, temperature=0.7)
            assert got_cl.dtype == torch.float32 and got_cl.is_contiguous()
            if W % 4 == 0:
                assert torch.equal(got, got_cl), (C, H, W)
            else:                # (the planar source took torch ops there, the channels-last one the kernel)
                K.assert_close(got_cl, want, f"{group} {activation} channels_last C={C} {H}x{W} {red}")


def test_deaugment_is_one_native_call_and_allocates_only_its_result(dev):
    from pytorch_toolbelt_amd import _native as N
    from pytorch_toolbelt_amd.inference import tta

    y = K.logits((8 * 4, 4, 256, 256), torch.bfloat16, 1).to(dev)
    for t in (y, y.contiguous(memory_format=CL)):
        for act in K.ACTIVATIONS:
            tta.d4_image_deaugment(t, activation=act)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before, calls = torch.cuda.max_memory_allocated(), N.calls
            out = tta.d4_image_deaugment(t, activation=act)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - before
            assert N.calls == calls + 1
            # the float32 result (1/8 of the batch's elements) and nothing of the batch's size -- a probability tensor would be 8 x that
            assert out.numel() * 4 <= peak < 2 * out.numel() * 4 and peak < t.numel() * t.element_size(), (peak, out.numel())


# ------------------------------------------------------------------------------------------------ incremental merger
def _feed(m, fed, dev, group, red, act, temp, layout=None, single=False):
    for y, crops in fed:
        y = y.to(dev)
        if layout is not None:
            y = y.contiguous(memory_format=layout)
        if group is not None:
            m.integrate_batch_deaugment(y, crops, group=group, reduction=red, activation=act, temperature=temp)
        elif single:
            for t, c in zip(y, crops):
                m.accumulate_single(t, c, activation=act, temperature=temp)
        else:
            m.integrate_batch(y, crops, activation=act, temperature=temp)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("activation", K.ACTIVATIONS)
@pytest.mark.parametrize("shape,tile,step,C,groups", [
    ((300, 420), 128, 64, 4, (None, "d4", "flips")),             # vector path, 50 % overlap: four covering tiles
    ((256, 256), 64, 16, 5, (None, "d4")),                       # 16-fold cover: launch groups are split; C = 5
    ((130, 170), (52, 36), (20, 12), 3, (None, "fliplr", "d2")),   # ragged chunks, non-square tiles
])
def test_incremental_merger(shape, tile, step, C, groups, activation, dtype, dev):
    from pytorch_toolbelt_amd import _native as N
    from pytorch_toolbelt_amd.inference import tta

    s = _slicer(shape, tile, step)
    for gi, group in enumerate(groups):
        red = K.REDUCTIONS[gi % 3]
        m, m_cl, m_two = (_merger(s, C, dev, auto_plan=False) for _ in range(3))
        for image in range(2):            # a second image after reset()
            fed = K.batches(s, C, group, dtype, 7, 10 * gi + image)
            want = K.model_image(s, C, fed, group, red, activation, 0.8)
            calls = N.calls
            _feed(m, fed, dev, group, red, activation, 0.8)
            assert N.calls == calls + len(fed)                 # one native call per batch: nothing in front of the merge launch
            assert m.mode == "incremental"
            got = m.merge()
            K.assert_close(got, want, f"incremental {shape} {group} {activation} image {image}")
            _feed(m_cl, fed, dev, group, red, activation, 0.8, layout=CL)
            assert torch.equal(m_cl.merge(), got)
            if group is not None:      # the fused merge == de-augment (fused activation), then merge
                for y, crops in fed:
                    fn = getattr(tta, f"{group}_image_deaugment")
                    m_two.integrate_batch(fn(y.to(dev), reduction=red, activation=activation, temperature=0.8), crops)
                assert torch.equal(m_two.merge(), got)
            elif image == 0:
                _feed(m_two, fed, dev, None, red, activation, 0.8, single=True)
                assert torch.equal(m_two.merge(), got)
            for mm in (m, m_cl, m_two):
                mm.reset()


def test_tiles_off_the_pixel_grid_take_the_fallback(dev):
    s = _slicer((77, 91), (25, 31), (11, 17))
    for act in K.ACTIVATIONS:
        fed = K.batches(s, 2, "fliplr", torch.float16, 5, 3)
        m = _merger(s, 2, dev, auto_plan=False)
        _feed(m, fed, dev, "fliplr", "mean", act, 1.0)
        K.assert_close(m.merge(), K.model_image(s, 2, fed, "fliplr", "mean", act), f"odd tiles {act}")


# ------------------------------------------------------------------------------------------------ deferred bands
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("activation", K.ACTIVATIONS)
@pytest.mark.parametrize("C", (4, 3))
def test_deferred_merger(C, activation, dtype, dev):
    s = _slicer((700, 900), 256, 128)
    for gi, group in enumerate(("d4", "fliplr", None)):
        red = K.REDUCTIONS[gi]
        fed = K.batches(s, C, group, dtype, 5, 20 + gi)
        for layout in (None, CL):
            d = _merger(s, C, dev, crops=s.crops, defer=True)
            inc = _merger(s, C, dev, auto_plan=False)
            for y, crops in fed:
                assert d.mode == "deferred bands"
                _feed(d, [(y, crops)], dev, group, red, activation, K.MAX_TEMPERATURE, layout=layout)
            assert d.mode == "deferred bands" and d._bands_done == len(d._bands.bands)
            _feed(inc, fed, dev, group, red, activation, K.MAX_TEMPERATURE, layout=layout)
            got = d.merge()
            assert torch.equal(got, inc.merge()), (group, layout)
        want = K.model_image(s, C, fed, group, red, activation, K.MAX_TEMPERATURE)
        K.assert_close(got, want, f"deferred C={C} {group} {activation}")
        if C > 1:
            K.assert_argmax(d.merge_crop(s, argmax=True, dtype=torch.uint8), want[:, s.margin_top:s.margin_top + s.image_height,
                                                                                  s.margin_left:s.margin_left + s.image_width],
                            f"deferred argmax C={C} {group} {activation}")


def test_change_of_activation_in_mid_image_gives_the_incremental_bits(dev):
    s = _slicer((700, 900), 256, 128)
    fed = K.batches(s, 4, "d4", torch.bfloat16, 5, 31)
    d = _merger(s, 4, dev, crops=s.crops, defer=True)
    inc = _merger(s, 4, dev, auto_plan=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, (y, crops) in enumerate(fed):
            act = "softmax" if i < 2 else "sigmoid"          # (before the first launch group goes out: the held batches are replayed)
            for m in (d, inc):
                m.integrate_batch_deaugment(y.to(dev), crops, group="d4", reduction="mean", activation=act)
            assert d.mode == ("deferred bands" if i < 2 else "incremental")
    assert torch.equal(d.merge(), inc.merge())


@pytest.mark.parametrize("activation", K.ACTIVATIONS)
def test_self_planned_second_image_defers_with_an_activation(activation, dev):
    from pytorch_toolbelt_amd.inference import tiles

    tiles.clear_auto_plans()
    s = _slicer((700, 900), 256, 128)
    fed = K.batches(s, 4, "d4", torch.float32, 5, 41)
    outs = []
    for image in range(2):
        m = _merger(s, 4, dev, auto_plan=True)
        ys = [y.to(dev) for y, _ in fed]
        for y, (_, crops) in zip(ys, fed):
            m.integrate_batch_deaugment(y, crops, group="d4", reduction="mean", activation=activation, temperature=0.9)
            assert m.mode == ("incremental" if image == 0 else "deferred bands")
        outs.append(m.merge())
    assert torch.equal(outs[0], outs[1])
    K.assert_close(outs[1], K.model_image(s, 4, fed, "d4", "mean", activation, 0.9), f"self-planned {activation}")
    tiles.clear_auto_plans()


def test_planned_blocks_merger_degrades_with_an_activation(dev):
    s = _slicer((300, 420), 128, 64)
    fed = K.batches(s, 4, "d4", torch.float16, 6, 51)
    p = _merger(s, 4, dev, crops=s.crops)
    inc = _merger(s, 4, dev, auto_plan=False)
    assert p.mode == "planned"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _feed(p, fed, dev, "d4", "gmean", "softmax", 1.0)
    assert p.mode == "incremental"
    _feed(inc, fed, dev, "d4", "gmean", "softmax", 1.0)
    assert torch.equal(p.merge(), inc.merge())


def test_lazy_handle_with_an_activation_is_evaluated_first(dev):
    from pytorch_toolbelt_amd.inference import tta

    s = _slicer((300, 420), 128, 64)
    fed = K.batches(s, 3, "fliplr", torch.float32, 6, 61)
    a, b = _merger(s, 3, dev, auto_plan=False), _merger(s, 3, dev, auto_plan=False)
    for y, crops in fed:
        y = y.to(dev)
        a.integrate_batch(tta.fliplr_image_deaugment(y), crops, activation="sigmoid")
        b.integrate_batch(tta.fliplr_image_deaugment(y) + 0, crops, activation="sigmoid")
    assert torch.equal(a.merge(), b.merge())


# ------------------------------------------------------------------------------------------------ saturation
@pytest.mark.parametrize("temperature", (1.0, 4.0))
@pytest.mark.parametrize("activation", K.ACTIVATIONS)
def test_saturated_logits_give_exact_zero_and_one(activation, temperature, dev):
    from pytorch_toolbelt_amd.inference import tta

    gen = torch.Generator().manual_seed(5)
    C = 4
    hot = torch.randint(0, C, (8 * 2, 1, 64, 64), generator=gen)
    y = torch.full((8 * 2, C, 64, 64), -100.0).scatter_(1, hot, 100.0)
    want = (y > 0).float()
    s = _slicer((128, 128), 64, 32)
    for layout in (None, CL):
        for group, V in (("d4", 8), (None, 1)):
            t = y[:V * 2].to(dev)
            t = t if layout is None else t.contiguous(memory_format=layout)
            p = tta.d4_image_deaugment(t, "sum", activation=activation, temperature=temperature) if group else None
            if p is not None:
                assert not torch.isnan(p).any() and set(p.unique().tolist()) <= {float(v) for v in range(9)}
        # through the mergers: channel 2 is hot everywhere, so the merged map is exactly sum(w) / sum(w) = 1 there and 0 elsewhere
        n = len(s.crops)
        tile = torch.full((n, C, 64, 64), -100.0)
        tile[:, 2] = 100.0
        tile = tile.to(dev)
        tile = tile if layout is None else tile.contiguous(memory_format=layout)
        for kw in (dict(auto_plan=False), dict(crops=s.crops, defer=True)):
            m = _merger(s, C, dev, **kw)
            m.integrate_batch(tile, s.crops, activation=activation, temperature=temperature)
            out = m.merge()
            assert not torch.isnan(out).any() and bool((out[2] == 1).all()) and bool((out[[0, 1, 3]] == 0).all())
