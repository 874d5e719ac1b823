"""CPU: channels_last_3d model outputs in the 3-D loop -- the 3-D entry points accept PTB_SRC_CHANNELS_LAST in their dtype argument and
keep their argument checks (every call here is refused or has B == 0, so no device is needed), ``_native.volume_layout`` classifies
5-D tensors while ``batch_layout`` stays 4-D-only, and the host forms give on a channels_last_3d twin what they give on the dense
batch (torch's own sum over 8 stacked views differs by an ulp between the two layouts, so the host forms reduce such a twin as the dense
batch)."""
import ctypes

import numpy as np
import pytest
import torch

from volume_defer_cases import cases

FAKE = ctypes.c_void_p(256)     # never dereferenced: every call below is refused by the argument checks or returns before a launch
F32, F16, BF16 = 0, 1, 2
CL = 0x200
EINVAL, EBOUNDS = -1, -4


def _lib():
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd import _native as N

    return N, N.load()


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _masks(*v):
    return (ctypes.c_int * len(v))(*v)


def _reduce(lib, src=FAKE, dtype=F32, B=0, C=4):
    return lib.ptb_volume_mirror_reduce(src, dtype, FAKE, 2, _masks(0, 7), 1, B, C, 4, 4, 4, None)


def _acc(lib, tiles=FAKE, dtype=F32, zs=None, B=0, C=4):
    zs = zs if zs is not None else _i64(0)
    return lib.ptb_volume_mirror_accumulate(FAKE, FAKE, FAKE, tiles, dtype, 2, _masks(0, 7), 1, zs, _i64(0), _i64(0), B, C, 4, 4, 4, 8, 8, 8, None)


def test_flag_value():
    N, _ = _lib()
    assert N.SRC_CHANNELS_LAST == CL


@pytest.mark.parametrize("dtype", [F32, F16, BF16])
def test_reduce_and_accumulate_accept_the_flag(dtype):
    _, lib = _lib()
    assert _reduce(lib, dtype=dtype | CL) == 0
    assert _acc(lib, dtype=dtype | CL) == 0
    assert _reduce(lib, dtype=dtype) == 0 and _acc(lib, dtype=dtype) == 0


def test_argument_checks_keep_their_codes_with_the_flag():
    _, lib = _lib()
    for call in (_reduce, _acc):
        assert call(lib, dtype=3 | CL) == EINVAL            # an unknown dtype
        assert call(lib, dtype=7 | CL) == EINVAL
        assert call(lib, dtype=0x100 | CL) == EINVAL        # PTB_ROUND_SRC has no meaning here
    assert _reduce(lib, src=None, dtype=F32 | CL) == EINVAL
    assert _acc(lib, tiles=None, dtype=F32 | CL) == EINVAL
    for dtype in (F32, F32 | CL, BF16 | CL):                # a roi outside the accumulator, with the flag as without it
        assert _acc(lib, dtype=dtype, zs=_i64(5), B=1) == EBOUNDS
        assert _acc(lib, dtype=dtype, zs=_i64(-1), B=1) == EBOUNDS


def test_the_bit_copy_refuses_the_flag():
    _, lib = _lib()
    for in_is_batch in (0, 1):
        assert lib.ptb_volume_mirror(FAKE, F32, FAKE, 2, _masks(0, 7), in_is_batch, 0, 4, 4, 4, 4, None) == 0
        for dtype in (F32, F16, BF16):
            assert lib.ptb_volume_mirror(FAKE, dtype | CL, FAKE, 2, _masks(0, 7), in_is_batch, 0, 4, 4, 4, 4, None) == EINVAL


def test_plan_submit_refuses_an_unknown_dtype_with_the_flag():
    N, lib = _lib()
    starts = [_i64(0), _i64(0), _i64(0)]
    plan = ctypes.c_void_p()
    assert lib.ptb_volume_plan_create(*starts, 1, 4, 4, 4, 4, 4, 4, 4, _i64(0, 0, 0, 4, 4, 4), 0, 0, ctypes.byref(plan)) > 0
    try:
        for dtype in (3 | CL, 0x100 | CL):
            assert lib.ptb_volume_plan_submit(plan, 0, 1, FAKE, 256, 0, dtype, 0, None, 0, FAKE, FAKE, None) == EINVAL
        # a known dtype with the flag passes the dtype check and stops where the call without it stops: no table uploaded yet
        assert lib.ptb_volume_plan_submit(plan, 0, 1, FAKE, 256, 0, F32 | CL, 0, None, 0, FAKE, FAKE, None) == \
            lib.ptb_volume_plan_submit(plan, 0, 1, FAKE, 256, 0, F32, 0, None, 0, FAKE, FAKE, None) == EINVAL
    finally:
        lib.ptb_volume_plan_destroy(plan)


# ------------------------------------------------------------------------------------------------ the classifier
def _cl(t):
    return t.contiguous(memory_format=torch.channels_last_3d)


def test_volume_layout():
    N, _ = _lib()
    dense = torch.rand(6, 4, 3, 5, 7)
    assert N.volume_layout(dense) == N.LAYOUT_DENSE
    assert N.volume_layout(dense[2:5]) == N.LAYOUT_DENSE
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        y = _cl(dense.to(dtype))
        assert not y.is_contiguous()
        assert N.volume_layout(y) == N.LAYOUT_CHANNELS_LAST
        assert N.volume_layout(y[2:5]) == N.LAYOUT_CHANNELS_LAST          # a slice of the batch dimension
        assert N.volume_layout(y[:1]) == N.LAYOUT_CHANNELS_LAST
    # the two formats coincide: dense
    assert N.volume_layout(_cl(torch.rand(3, 1, 3, 5, 7))) == N.LAYOUT_DENSE
    assert N.volume_layout(_cl(torch.rand(3, 4, 1, 1, 1))) == N.LAYOUT_DENSE
    y = _cl(dense)
    for other in (y[:, 1:3], y[:, :, ::2], y[:, :, :, 1:], y[..., :5], dense[:, 1:3], dense[..., ::2], dense.transpose(3, 4),
                  _cl(dense[:1]).expand(4, -1, -1, -1, -1), torch.rand(4, 3, 5, 7).contiguous(memory_format=torch.channels_last),
                  torch.rand(4, 3, 5, 7), torch.rand(2, 2, 4, 3, 5, 7)):
        assert N.volume_layout(other) == N.LAYOUT_OTHER, (tuple(other.shape), other.stride())
    # the 4-D classifiers stay 4-D-only
    assert N.batch_layout(y) == N.LAYOUT_OTHER and not N.dense_or_channels_last(y)
    assert N.batch_layout(dense) == N.LAYOUT_DENSE


# ------------------------------------------------------------------------------------------------ the host path is unchanged
@pytest.mark.parametrize("reduction", ["mean", "gmean", "sum", None])
def test_host_deaugment_on_a_channels_last_twin(reduction):
    from pytorch_toolbelt_amd.inference.tta_3d import mirror_volume_deaugment

    dense = torch.rand(8 * 2, 3, 4, 5, 6) * 0.8 + 0.1
    y = _cl(dense)
    before = y.clone()
    for mirror in ("dhw", "h", "dw"):
        V = {"dhw": 8, "h": 2, "dw": 4}[mirror]
        got, want = mirror_volume_deaugment(y[:V * 2], mirror, reduction), mirror_volume_deaugment(dense[:V * 2], mirror, reduction)
        assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(y, before) and _layout_is_kept(y)


def _layout_is_kept(y):
    return y.is_contiguous(memory_format=torch.channels_last_3d) and not y.is_contiguous()


@pytest.mark.parametrize("name", ["half_overlap", "off_grid", "gap"])
@pytest.mark.parametrize("defer", [False, True])
def test_host_merger_on_a_channels_last_twin(name, defer):
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumeMerger

    case = cases()[name]
    crops, n, C = case["crops"], len(case["crops"]), 3
    spec = dict(crop=case["window"], layout="dhwc", dtype=torch.float32)
    for mirror in (None, "hw", "dhw"):
        V = {None: 1, "hw": 4, "dhw": 8}[mirror]
        kwargs = dict(crops=crops, defer=True, result=spec) if defer else {}
        mergers = [VolumeMerger(case["shape"], C, case["weight"], device="cpu", **kwargs) for _ in range(2)]
        gen = torch.Generator().manual_seed(3)
        for b0 in range(0, n, 3):
            rois = crops[b0:b0 + 3]
            dense = torch.rand((V * len(rois), C) + case["tile"], generator=gen) * 0.8 + 0.1
            for m, batch in zip(mergers, (dense, _cl(dense))):
                if mirror is None:
                    m.integrate_batch(batch, rois)
                else:
                    m.integrate_batch_deaugment(batch, rois, mirror=mirror, reduction="mean")
        want, got = (m.merge_crop(**spec) for m in mergers)
        assert np.array_equal(got.numpy().view(np.int32), want.numpy().view(np.int32))
