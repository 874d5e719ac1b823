"""``activation=`` / ``temperature=`` of the 3-D mirror de-augmentation and tile merges without a GPU: the host paths against the float64
model, the argument errors, the validation of the three new entry points, and ``activation=None`` as the call without the keyword."""
import ctypes

import numpy as np
import pytest
import torch

import volume_activation_cases as VA
from volume_defer_cases import cases

CASES = cases()


def _merger(case, channels, **kw):
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumeMerger

    return VolumeMerger(case["shape"], channels, case["weight"], device="cpu", **kw)


@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
@pytest.mark.parametrize("reduction", VA.REDUCTIONS)
def test_host_deaugment_matches_the_model(activation, reduction):
    from pytorch_toolbelt_amd.inference.tta_3d import apply_activation, mirror_volume_deaugment

    # temperatures of at most 1 keep z = x * t inside the [-3, 3] the tolerance was worked out for (logodd cancels in 1 - p beyond it)
    for dtype, mirror, temperature in ((torch.float32, "dhw", 1.0), (torch.bfloat16, "dh", 0.5), (torch.float16, "w", 0.75)):
        y = VA.logits((2 ** len(mirror) * 2, 3, 5, 6, 7), dtype, seed=3)      # B = 2
        got = mirror_volume_deaugment(y, mirror, reduction, activation=activation, temperature=temperature)
        assert got.dtype == torch.float32
        VA.assert_close(got, VA.deaugment64(y, mirror, reduction, activation, temperature), (activation, reduction, dtype, mirror))
        assert torch.equal(got, mirror_volume_deaugment(apply_activation(y, activation, temperature), mirror, reduction))
    # a channels_last_3d host batch reduces as its dense copy does
    y = VA.logits((4, 4, 5, 6, 7), torch.float32, seed=4)
    cl = y.contiguous(memory_format=torch.channels_last_3d)
    assert torch.equal(mirror_volume_deaugment(cl, "dh", reduction, activation=activation), mirror_volume_deaugment(y, "dh", reduction, activation=activation))


@pytest.mark.parametrize("activation", ["sigmoid", "softmax"])
def test_unfusable_reductions_apply_the_activation_with_torch_ops(activation):
    from pytorch_toolbelt_amd.inference.tta_3d import apply_activation, mirror_volume_deaugment

    y = VA.logits((4, 3, 4, 5, 6), torch.float32, seed=5)
    stack = mirror_volume_deaugment(y, "dh", None, activation=activation, temperature=0.7)
    assert stack.shape == (4, 1, 3, 4, 5, 6)
    assert torch.equal(stack, mirror_volume_deaugment(apply_activation(y, activation, 0.7), "dh", None))
    got = mirror_volume_deaugment(y, "dh", torch.amax, activation=activation, temperature=0.7)
    assert torch.equal(got, stack.amax(dim=0))


@pytest.mark.parametrize("name", ["half_overlap", "off_grid", "gap"])
@pytest.mark.parametrize("activation, mirror, reduction", [("softmax", None, "mean"), ("softmax", "dhw", "gmean"), ("sigmoid", "dw", "logodd"),
                                                           ("sigmoid", None, "mean")])
def test_host_merger_matches_the_model(name, activation, mirror, reduction):
    case = CASES[name]
    fed = VA.batches(case, 4, mirror, torch.float32, 3, seed=11)
    want = VA.merge64(case, VA.model_tiles(fed, mirror, reduction, activation, 0.75))
    spec = dict(crop=case["window"], layout="cdhw", dtype=torch.float32, argmax=False)
    plain, deferred = _merger(case, 4), _merger(case, 4, crops=case["crops"], defer=True, result=spec)
    for m in (plain, deferred):
        for y, rois in fed:
            if mirror is None:
                m.integrate_batch(y, rois, activation=activation, temperature=0.75)
            else:
                m.integrate_batch_deaugment(y, rois, mirror, reduction, activation=activation, temperature=0.75)
    VA.assert_close(plain.merge(), want, (name, activation, "merge"))
    VA.assert_close(deferred.merge_crop(**spec), VA.window_of(case, want), (name, activation, "deferred"))
    labels = plain.merge_crop(case["window"], argmax=True, dtype=torch.uint8)
    VA.assert_argmax(labels, VA.window_of(case, want), (name, activation, "argmax"))


def test_float64_accumulators_and_accumulate_single():
    from pytorch_toolbelt_amd.inference.tiles_3d import HostBackedVolumeMerger

    case = CASES["off_grid"]
    fed = VA.batches(case, 3, None, torch.float32, 1, seed=12)
    want = VA.merge64(case, VA.model_tiles(fed, None, "mean", "softmax"))
    m = _merger(case, 3, dtype=torch.float64)
    assert type(m) is HostBackedVolumeMerger
    for y, rois in fed:
        m.accumulate_single(y[0], rois[0], activation="softmax")
    VA.assert_close(m.merge(), want, "float64 accumulators", tol=1e-6)     # float32 probabilities, float64 sums


def test_argument_errors():
    from pytorch_toolbelt_amd.inference.tta_3d import mirror_volume_deaugment

    case = CASES["single_tile"]
    y = VA.logits((2, 2) + case["tile"], torch.float32, seed=1)
    rois = case["crops"][:1]
    m = _merger(case, 2)
    for bad in ("relu", "Softmax", 1, True):
        with pytest.raises(ValueError, match="activation"):
            mirror_volume_deaugment(y, "w", "mean", activation=bad)
        with pytest.raises(ValueError, match="activation"):
            m.integrate_batch(y[:1], rois, activation=bad)
        with pytest.raises(ValueError, match="activation"):
            m.integrate_batch_deaugment(y, rois, "w", "mean", activation=bad)
        with pytest.raises(ValueError, match="activation"):
            m.accumulate_single(y[0], rois[0], activation=bad)
    for bad in (float("nan"), float("inf"), -float("inf"), None, "1"):
        with pytest.raises(ValueError, match="temperature"):
            mirror_volume_deaugment(y, "w", "mean", activation="sigmoid", temperature=bad)
        with pytest.raises(ValueError, match="temperature"):
            m.integrate_batch(y[:1], rois, activation="softmax", temperature=bad)
        with pytest.raises(ValueError, match="temperature"):
            m.integrate_batch_deaugment(y, rois, "w", "mean", activation="softmax", temperature=bad)
    for reduction in (None, torch.amax):        # the merge keeps refusing what it cannot fuse, with or without an activation
        with pytest.raises(ValueError, match="cannot be fused"):
            m.integrate_batch_deaugment(y, rois, "w", reduction, activation="softmax")
    with pytest.raises(TypeError):              # keyword-only
        m.integrate_batch(y[:1], rois, "softmax")
    assert float(m.norm_mask.abs().max()) == 0.0           # nothing was blended by a refused call


def test_deferred_host_merger_keeps_one_activation_per_image():
    case = CASES["half_overlap"]
    fed = VA.batches(case, 2, None, torch.float32, 2, seed=2)
    m = _merger(case, 2, crops=case["crops"], defer=True)
    m.integrate_batch(fed[0][0], fed[0][1], activation="softmax")
    for kw in (dict(activation="sigmoid"), dict(activation="softmax", temperature=2.0), dict()):
        with pytest.raises(RuntimeError, match="activation"):
            m.integrate_batch(fed[1][0], fed[1][1], **kw)
    m.reset()
    m.integrate_batch(fed[0][0], fed[0][1], activation="sigmoid", temperature=2.0)


def test_activation_none_is_the_call_without_the_keyword():
    from pytorch_toolbelt_amd.inference.tta_3d import mirror_volume_deaugment

    case = CASES["off_grid"]
    fed = VA.batches(case, 3, "dh", torch.float16, 4, seed=6)
    y = fed[0][0]
    a, b = mirror_volume_deaugment(y, "dh", "gmean"), mirror_volume_deaugment(y, "dh", "gmean", activation=None, temperature=3.0)
    assert a.dtype == b.dtype == torch.float16 and torch.equal(a.view(torch.int16), b.view(torch.int16))
    with_kw, without = _merger(case, 3), _merger(case, 3)
    for y, rois in fed:
        without.integrate_batch_deaugment(y, rois, "dh", "mean")
        with_kw.integrate_batch_deaugment(y, rois, "dh", "mean", activation=None, temperature=3.0)
        without.integrate_batch(y[:len(rois)], rois)
        with_kw.integrate_batch(y[:len(rois)], rois, activation=None)
        without.accumulate_single(y[0], rois[0])
        with_kw.accumulate_single(y[0], rois[0], activation=None)
    assert torch.equal(with_kw.volume, without.volume) and torch.equal(with_kw.norm_mask, without.norm_mask)


def test_new_entry_points_validate_without_gpu():
    """Arguments are validated before anything touches the device, so these calls are safe without one."""
    from pytorch_toolbelt_amd import _native as N

    lib = N.load()
    assert (N.ACT_NONE, N.ACT_SIGMOID, N.ACT_SOFTMAX) == (0, 1, 2)
    one = N.int_array([0])
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    z = N.i64_array([0])
    # ptb_volume_mirror_reduce_act(src, dtype, dst, nviews, masks, reduction, B, C, D, H, W, activation, temperature, stream)
    assert lib.ptb_volume_mirror_reduce_act(None, N.F32, p, 1, one, N.RED_MEAN, 1, 1, 2, 2, 2, N.ACT_SIGMOID, 1.0, None) == -1
    assert lib.ptb_volume_mirror_reduce_act(p, N.F32, None, 1, one, N.RED_MEAN, 1, 1, 2, 2, 2, N.ACT_SIGMOID, 1.0, None) == -1
    assert lib.ptb_volume_mirror_reduce_act(p, N.F32, p, 1, one, N.RED_MEAN, 1, 1, 2, 2, 2, 3, 1.0, None) == -1
    assert lib.ptb_volume_mirror_reduce_act(p, N.F32, p, 1, one, N.RED_MEAN, 1, 1, 2, 2, 2, -1, 1.0, None) == -1
    assert lib.ptb_volume_mirror_reduce_act(p, N.F32, p, 1, one, N.RED_MEAN, 1, 1, 2, 2, 2, N.ACT_SOFTMAX, float("nan"), None) == -1
    assert lib.ptb_volume_mirror_reduce_act(p, N.F32, p, 1, one, N.RED_MEAN, 1, 1, 2, 2, 2, N.ACT_SOFTMAX, float("inf"), None) == -1
    assert lib.ptb_volume_mirror_reduce_act(p, 7, p, 1, one, N.RED_MEAN, 1, 1, 2, 2, 2, N.ACT_SOFTMAX, 1.0, None) == -1
    assert lib.ptb_volume_mirror_reduce_act(p, N.F32, p, 1, one, 9, 1, 1, 2, 2, 2, N.ACT_SOFTMAX, 1.0, None) == -1
    assert lib.ptb_volume_mirror_reduce_act(p, N.F32, p, 0, one, N.RED_MEAN, 1, 1, 2, 2, 2, N.ACT_SOFTMAX, 1.0, None) == -1
    assert lib.ptb_volume_mirror_reduce_act(p, N.F32, p, 1, one, N.RED_MEAN, 1, 17, 2, 2, 2, N.ACT_SOFTMAX, 1.0, None) == N.PTB_EUNSUPPORTED
    assert lib.ptb_volume_mirror_reduce_act(p, N.F32, p, 1, one, N.RED_MEAN, 0, 17, 2, 2, 2, N.ACT_SIGMOID, 1.0, None) == 0       # B = 0: nothing to do
    # ptb_volume_mirror_accumulate_act(volume, norm, weight, tiles, in_dtype, nviews, masks, reduction, zs, ys, xs, B, C, d, h, w, D, H, W, act, t, stream)
    tail = (1, 1, 2, 2, 2, 4, 4, 4)
    assert lib.ptb_volume_mirror_accumulate_act(None, p, p, p, N.F32, 1, one, N.RED_SUM, z, z, z, *tail, N.ACT_SIGMOID, 1.0, None) == -1
    assert lib.ptb_volume_mirror_accumulate_act(p, p, p, None, N.F32, 1, one, N.RED_SUM, z, z, z, *tail, N.ACT_SIGMOID, 1.0, None) == -1
    assert lib.ptb_volume_mirror_accumulate_act(p, p, p, p, N.F32, 1, one, N.RED_SUM, z, z, z, *tail, 5, 1.0, None) == -1
    assert lib.ptb_volume_mirror_accumulate_act(p, p, p, p, N.F32, 1, one, N.RED_SUM, z, z, z, *tail, N.ACT_SIGMOID, float("nan"), None) == -1
    assert lib.ptb_volume_mirror_accumulate_act(p, p, p, p, N.F32, 1, one, N.RED_SUM, N.i64_array([3]), z, z, *tail, N.ACT_SIGMOID, 1.0, None) == -4
    assert lib.ptb_volume_mirror_accumulate_act(p, p, p, p, N.F32, 1, one, N.RED_SUM, z, z, z, 1, 17, 2, 2, 2, 4, 4, 4, N.ACT_SOFTMAX, 1.0,
                                                None) == N.PTB_EUNSUPPORTED
    # ptb_volume_plan_submit_act(plan, pos, B, batch, tile_stride, view_stride, in_dtype, nviews, masks, reduction, weight, out, act, t, stream)
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumePlan

    case = CASES["single_tile"]
    for channels, act, want in ((2, N.ACT_SOFTMAX, -1), (17, N.ACT_SOFTMAX, N.PTB_EUNSUPPORTED), (17, N.ACT_SIGMOID, -1)):
        plan = VolumePlan(case["crops"], case["tile"], case["shape"], channels)
        args = (plan.handle, 0, 1, p, 8, 8, N.F32, 0, None, 0, p, p)
        assert lib.ptb_volume_plan_submit_act(None, *args[1:], act, 1.0, None) == -1
        assert lib.ptb_volume_plan_submit_act(*args, 3, 1.0, None) == -1
        assert lib.ptb_volume_plan_submit_act(*args, act, float("nan"), None) == -1
        assert lib.ptb_volume_plan_submit_act(*args[:3], None, *args[4:], act, 1.0, None) == -1
        assert lib.ptb_volume_plan_submit_act(*args, act, 1.0, None) == want            # (-1: no table uploaded yet, nothing can be launched)
        plan.close()
