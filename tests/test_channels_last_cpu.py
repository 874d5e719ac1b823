"""Channels-last model outputs (PTB_SRC_CHANNELS_LAST), the parts that need no GPU: the ABI flag and its argument validation, the batch
classifier, and a guard that the host path -- which never cared about strides -- still gives the dense result for channels-last tensors."""
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value_matches_the_header():
    from pytorch_toolbelt_amd import _native as N

    assert N.SRC_CHANNELS_LAST == 0x200
    header = open(os.path.join(ROOT, "include", "ptb_hip.h")).read()
    m = re.search(r"#define\s+PTB_SRC_CHANNELS_LAST\s+(\S+)", header)
    assert m and int(m.group(1), 0) == N.SRC_CHANNELS_LAST
    assert N.SRC_CHANNELS_LAST & N.ROUND_SRC == 0 and N.SRC_CHANNELS_LAST & N.DTYPE_MASK == 0
    assert N._ERR[-5] and N._ERR[-6]                     # PTB_EFRESH / PTB_EHELD have texts too


def test_argument_validation_without_gpu():
    """Entry points validate arguments before touching the device, so these calls are safe without a GPU.  Nothing here gets as far as a
    launch: every call fails its checks (or has B == 0)."""
    from pytorch_toolbelt_amd import _native as N

    lib = N.load()
    CL = N.SRC_CHANNELS_LAST
    views = N.int_array([0] * 8)
    xs = N.i64_array([0])
    ys = N.i64_array([0])
    one = 16        # any non-NULL address: the checks below never dereference it
    # the flag with an unknown dtype is PTB_EINVAL, as an unknown dtype is without it
    assert lib.ptb_deaug_reduce_t(one, 7, one, 8, views, 1, 1, 4, 8, 8, None) == -1
    assert lib.ptb_deaug_reduce_t(one, 7 | CL, one, 8, views, 1, 1, 4, 8, 8, None) == -1
    assert lib.ptb_deaug_accumulate_t(one, None, one, one, 7 | CL, 8, views, 1, xs, ys, 1, 4, 8, 8, 8, 8, None, 0, None) == -1
    assert lib.ptb_accumulate_planned2(one, one, one, one, one, 7 | CL, 8, views, 1, xs, ys, 1, 4, 64, 64, 64, 64, None, 32, one, one, 0, None) == -1
    assert lib.ptb_merge_band(one, one, one, one, one, 7 | CL, 8, None, 1, None, None, 1, 4, 8, 8, 8, 8, 0, 8, None) == -1
    # a NULL source
    for dt in (N.F32 | CL, N.F16 | CL, N.BF16 | CL | N.ROUND_SRC):
        assert lib.ptb_deaug_reduce_t(None, dt & ~N.ROUND_SRC, one, 8, views, 1, 1, 4, 8, 8, None) == -1
        assert lib.ptb_deaug_accumulate_t(one, None, one, None, dt, 8, views, 1, xs, ys, 1, 4, 8, 8, 8, 8, None, 0, None) == -1
        assert lib.ptb_accumulate_planned2(one, one, one, one, None, dt, 8, views, 1, xs, ys, 1, 4, 64, 64, 64, 64, None, 32, one, one, 0, None) == -1
    # C < 1
    assert lib.ptb_deaug_reduce_t(one, N.F32 | CL, one, 8, views, 1, 1, 0, 8, 8, None) == -1
    assert lib.ptb_deaug_accumulate_t(one, None, one, one, N.F32 | CL, 8, views, 1, xs, ys, 1, 0, 8, 8, 8, 8, None, 0, None) == -1
    assert lib.ptb_accumulate_planned2(one, one, one, one, one, N.F32 | CL, 8, views, 1, xs, ys, 1, 0, 64, 64, 64, 64, None, 32, one, one, 0, None) == -1
    # argument checks keep their order: a tile outside the accumulator is PTB_EBOUNDS with the flag as without it
    far = N.i64_array([100])
    for dt in (N.F32, N.F32 | CL):
        assert lib.ptb_deaug_accumulate_t(one, None, one, one, dt, 8, views, 1, far, ys, 1, 4, 8, 8, 8, 8, None, 0, None) == -4
    # an empty batch is fine (B == 0: nothing is read, nothing launched)
    assert lib.ptb_deaug_reduce_t(one, N.BF16 | CL, one, 8, views, 1, 0, 4, 8, 8, None) == 0
    # a band plan without an uploaded table refuses the submit before it looks at the layout
    assert lib.ptb_band_plan_submit(None, 0, 1, one, 256, 256, N.F32 | CL, 1, views, 0, one, one, one, None) == -1


def test_batch_classifier():
    from pytorch_toolbelt_amd import _native as N

    D, CLAST, OTHER = N.LAYOUT_DENSE, N.LAYOUT_CHANNELS_LAST, N.LAYOUT_OTHER
    x = torch.zeros(6, 4, 8, 12)
    cl = x.contiguous(memory_format=torch.channels_last)
    assert N.batch_layout(x) == D and N.layout_flag(x) == 0 and N.dense_or_channels_last(x)
    assert N.batch_layout(cl) == CLAST and N.layout_flag(cl) == N.SRC_CHANNELS_LAST and N.dense_or_channels_last(cl)
    assert cl.stride() == (8 * 12 * 4, 1, 12 * 4, 4)
    # where the two formats coincide the tensor is dense: today's path serves it
    assert N.batch_layout(torch.zeros(6, 1, 8, 12).contiguous(memory_format=torch.channels_last)) == D
    assert N.batch_layout(torch.zeros(6, 4, 1, 1).contiguous(memory_format=torch.channels_last)) == D
    # half precision, slices of the batch dimension
    assert N.batch_layout(cl.half()) == CLAST and N.batch_layout(cl.bfloat16()[2:5]) == CLAST
    # anything else is copied as before
    assert N.batch_layout(cl[:, :2]) == OTHER and not N.dense_or_channels_last(cl[:, :2])       # channel slice of a channels-last batch
    assert N.batch_layout(x[:, :2]) == OTHER                                                    # ... and of a dense one
    assert N.batch_layout(x.transpose(2, 3)) == OTHER
    assert N.batch_layout(cl[:, :, ::2]) == OTHER
    assert N.batch_layout(torch.zeros(1, 4, 8, 12).expand(6, 4, 8, 12)) == OTHER
    # 3-D / 5-D tensors are never channels-last here (channels_last_3d is out of scope)
    assert N.batch_layout(torch.zeros(4, 8, 12).permute(1, 2, 0)) == OTHER
    v = torch.zeros(2, 4, 6, 8, 12)
    assert N.batch_layout(v) == D and N.batch_layout(v.contiguous(memory_format=torch.channels_last_3d)) == OTHER


def test_host_path_is_unchanged_for_channels_last_tensors():
    """CPU tensors take the torch-op path, which never looked at strides: a guard that it still equals the dense call."""
    from pytorch_toolbelt_amd.inference import tta
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer, TileMerger

    g = torch.Generator().manual_seed(3)
    slicer = ImageSlicer((150, 130, 3), 64, 32, weight="pyramid")
    n, C = len(slicer.crops), 4
    y = torch.rand((8 * n, C, 64, 64), generator=g) + 0.1
    y_cl = y.contiguous(memory_format=torch.channels_last)
    assert not y_cl.is_contiguous()
    for red in ("mean", "gmean"):
        dense = tta.d4_image_deaugment(y, reduction=red)
        assert torch.equal(tta.d4_image_deaugment(y_cl, reduction=red), dense)
    assert torch.equal(tta.fliplr_labels_deaugment(y_cl[:2 * n]), tta.fliplr_labels_deaugment(y[:2 * n]))
    a = TileMerger(slicer.target_shape, C, slicer.weight)
    b = TileMerger(slicer.target_shape, C, slicer.weight)
    for b0 in range(0, n, 5):
        a.integrate_batch(y[b0:min(n, b0 + 5)], slicer.crops[b0:b0 + 5])
        b.integrate_batch(y_cl[b0:min(n, b0 + 5)], slicer.crops[b0:b0 + 5])
    assert torch.equal(a.merge(), b.merge()) and np.array_equal(a.norm_mask.numpy(), b.norm_mask.numpy())
