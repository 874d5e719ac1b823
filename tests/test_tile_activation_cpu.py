"""``activation=`` / ``temperature=`` of the 2-D de-augmentations and the tile mergers without a GPU: the float64 model of
tests/tile_activation_cases.py against plain torch, the host paths against the model, argument errors, the unchanged default, autograd
through the torch-op fallback."""
import numpy as np
import pytest
import torch

import tile_activation_cases as K

from pytorch_toolbelt_amd.inference import _lazy, tta
from pytorch_toolbelt_amd.inference.tiles import ImageSlicer, TileMerger

# (image, tile, step, channels): the geometries of the GPU tests' mergers
GEOMETRIES = (((300, 420), 128, 64, 4), ((256, 256), 64, 16, 5), ((130, 170), (52, 36), (20, 12), 3), ((700, 900), 256, 128, 4), ((700, 900), 256, 128, 3))


def _slicer(shape, tile, step):
    return ImageSlicer(tuple(shape) + (3,), tile, step, weight="pyramid")


@pytest.mark.parametrize("group", K.GROUPS)
def test_model_views_are_the_deaugmentation(group):
    y = K.logits((len(tta.DEAUGMENT_VIEWS[group]) * 2, 3, 12, 12), torch.float32, 1)
    for act in K.ACTIVATIONS:
        p = K.activate64(y, act, 1.5)
        assert torch.allclose(p, (y.double() * 1.5).sigmoid() if act == "sigmoid" else (y.double() * 1.5).softmax(1), rtol=0, atol=1e-15)
        for red in K.REDUCTIONS:
            want = getattr(tta, f"{group}_image_deaugment")(p, reduction=red)      # the host path, in float64
            got = K.deaugment64(y, group, red, act, 1.5)
            assert float((torch.as_tensor(want) - got).abs().max()) <= 1e-9, (group, act, red)


def test_model_merge_is_the_sequential_blend():
    s = _slicer((130, 170), (52, 36), (20, 12))
    fed = K.batches(s, 3, None, torch.float32, 5, 3)
    want = K.model_image(s, 3, fed, None, "mean", "softmax")
    m = TileMerger(s.target_shape, 3, s.weight, dtype=torch.float64)
    for y, crops in fed:
        m.integrate_batch(y.double().softmax(1), crops)
    assert float((m.merge() - want).abs().nan_to_num(0.0).max()) <= 1e-12


@pytest.mark.parametrize("shape,tile,step,C", GEOMETRIES)
def test_near_ties_of_the_cases_stay_under_the_bound(shape, tile, step, C):
    s = _slicer(shape, tile, step)
    for group in (None, "fliplr") if isinstance(tile, tuple) else (None, "fliplr", "d4"):
        fed = K.batches(s, C, group, torch.float32, 8, 11)
        for act in K.ACTIVATIONS:
            share = K.near_tie_share(K.model_image(s, C, fed, group, "mean", act))
            assert share <= K.ARGMAX_SKIP, (group, act, share)


@pytest.mark.parametrize("activation", K.ACTIVATIONS)
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_host_deaugment_and_merger_against_the_model(activation, dtype):
    for group in ("fliplr", "d4"):
        y = K.logits((len(tta.DEAUGMENT_VIEWS[group]) * 2, 5, 20, 20), dtype, 5)
        for red in K.REDUCTIONS:
            got = getattr(tta, f"{group}_image_deaugment")(y, reduction=red, activation=activation, temperature=0.7)
            assert type(got) is torch.Tensor and got.dtype == torch.float32
            K.assert_close(got, K.deaugment64(y, group, red, activation, 0.7), f"host {group} {red} {activation}")
    s = _slicer((130, 170), (52, 36), (20, 12))
    for group in (None, "d2"):
        fed = K.batches(s, 3, group, dtype, 4, 7)
        m = TileMerger(s.target_shape, 3, s.weight)
        assert m.mode == "host"
        for y, crops in fed:
            if group is None:
                m.integrate_batch(y, crops, activation=activation, temperature=2.0)
            else:
                m.integrate_batch_deaugment(y, crops, group=group, reduction="gmean", activation=activation, temperature=2.0)
        K.assert_close(m.merge(), K.model_image(s, 3, fed, group, "gmean", activation, 2.0), f"host merger {group} {activation}")
    m = TileMerger(s.target_shape, 3, s.weight)
    fed = K.batches(s, 3, None, dtype, 1, 9)
    for y, crops in fed:
        m.accumulate_single(y[0], crops[0], activation=activation)
    K.assert_close(m.merge(), K.model_image(s, 3, fed, None, "mean", activation), f"host accumulate_single {activation}")


def test_argument_errors():
    y = torch.zeros((8, 17, 8, 8))
    s = _slicer((64, 64), 32, 16)
    m = TileMerger(s.target_shape, 17, s.weight)
    t = torch.zeros((len(s.crops), 17, 32, 32))
    for call in (lambda **kw: tta.d4_image_deaugment(y, **kw), lambda **kw: tta.fliplr_image_deaugment(y, "gmean", **kw),
                 lambda **kw: m.integrate_batch(t, s.crops, **kw), lambda **kw: m.accumulate_single(t[0], s.crops[0], **kw),
                 lambda **kw: m.integrate_batch_deaugment(torch.cat([t, t]), s.crops, group="fliplr", **kw)):
        with pytest.raises(ValueError, match="activation must be"):
            call(activation="relu")
        for bad in (float("nan"), float("inf"), "1", None, True):
            with pytest.raises(ValueError, match="temperature"):
                call(activation="sigmoid", temperature=bad)
    with pytest.raises(TypeError):
        tta.d4_image_deaugment(y, "mean", "sigmoid")          # keyword-only


def test_softmax_above_16_channels_is_refused_on_the_fused_route_only(monkeypatch):
    from pytorch_toolbelt_amd.inference.tta_3d import _check_softmax_channels
    from pytorch_toolbelt_amd import _native as N

    with pytest.raises(NotImplementedError, match=r"softmax\(1\)"):
        _check_softmax_channels(N.ACT_SOFTMAX, 17, "d4_image_deaugment")
    _check_softmax_channels(N.ACT_SIGMOID, 17, "d4_image_deaugment")
    # a GPU merger refuses before anything is launched (the check is the mergers' own: no device is needed to see it raise)
    s = _slicer((64, 64), 32, 16)
    m = object.__new__(TileMerger)
    m.channels = 17
    with pytest.raises(NotImplementedError, match=r"softmax\(1\)"):
        TileMerger._activation(m, "softmax", 1.0, "TileMerger.integrate_batch")
    assert TileMerger._activation(m, "sigmoid", 1.0, "TileMerger.integrate_batch") == (N.ACT_SIGMOID, 1.0)
    # the host route applies torch's softmax to any number of channels
    y = K.logits((2, 17, 8, 8), torch.float32, 2)
    K.assert_close(tta.fliplr_image_deaugment(y, activation="softmax"), K.deaugment64(y, "fliplr", "mean", "softmax"), "host softmax C = 17")


def test_default_is_the_call_as_it_was():
    y = K.logits((8, 3, 8, 8), torch.float32, 4)
    a, b = tta.d4_image_deaugment(y), tta.d4_image_deaugment(y, activation=None, temperature=3.0)
    assert type(a) is type(b) and torch.equal(torch.as_tensor(a), torch.as_tensor(b))
    # where today's call hands out a lazy handle the default still does (the decision is _lazy.maybe_lazy's, reached with the same arguments)
    seen = []
    real = _lazy.maybe_lazy

    def spy(*args, **kw):
        seen.append((len(args), sorted(kw)))
        return real(*args, **kw)

    _lazy.maybe_lazy, keep = spy, _lazy.maybe_lazy
    try:
        tta.d4_image_deaugment(y)
        tta.d4_image_deaugment(y, activation=None)
        tta.d4_image_deaugment(y, activation="sigmoid")
    finally:
        _lazy.maybe_lazy = keep
    assert len(seen) == 2 and seen[0] == seen[1], seen          # the activated call never asks for a handle
    s = _slicer((64, 64), 32, 16)
    m1, m2 = TileMerger(s.target_shape, 3, s.weight), TileMerger(s.target_shape, 3, s.weight)
    t = K.logits((len(s.crops), 3, 32, 32), torch.float32, 6)
    m1.integrate_batch(t, s.crops)
    m2.integrate_batch(t, s.crops, activation=None)
    assert torch.equal(m1.merge(), m2.merge())


def test_autograd_through_the_fallback():
    y = K.logits((4, 3, 8, 8), torch.float32, 8).requires_grad_(True)
    out = tta.d2_image_deaugment(y, "mean", activation="softmax", temperature=0.5)
    assert out.requires_grad and out.dtype == torch.float32
    out.square().sum().backward()
    ref = y.detach().clone().requires_grad_(True)
    tta.d2_image_deaugment((ref * 0.5).softmax(1), "mean").square().sum().backward()
    assert torch.allclose(y.grad, ref.grad, rtol=0, atol=1e-7)
    # callable / None reductions take the same route
    stack = tta.fliplr_image_deaugment(y.detach(), None, activation="sigmoid")
    assert stack.shape == (2, 2, 3, 8, 8)
    got = tta.fliplr_image_deaugment(y.detach(), torch.amax, activation="sigmoid")
    assert torch.equal(got, stack.amax(dim=0))


def test_sharded_merger_names_the_unfused_form():
    from pytorch_toolbelt_amd.parallel import ShardedTileMerger

    for name in ("integrate_batch", "integrate_batch_deaugment"):
        with pytest.raises(NotImplementedError, match="apply_activation"):
            getattr(ShardedTileMerger, name)(object.__new__(ShardedTileMerger), None, None, activation="sigmoid")
