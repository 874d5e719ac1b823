"""CPU: mirror test-time augmentation of 3-D tiles -- ptb_volume_mirror / _mirror_reduce / _mirror_accumulate / ptb_volume_split_mirror
are declared and exported and refuse bad arguments before any launch, MIRROR_VIEWS follows its definition, split_device(mirror=)
refuses host tensors, and the host forms (tta_3d on CPU tensors, HostBackedVolumeMerger.integrate_batch_deaugment) equal the torch
expressions they stand for."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

FAKE = ctypes.c_void_p(256)     # never dereferenced: every call below is refused by the argument checks
NAMES = ("ptb_volume_mirror", "ptb_volume_mirror_reduce", "ptb_volume_mirror_accumulate", "ptb_volume_split_mirror")
FLIPS = {0: [], 1: [4], 2: [3], 3: [3, 4], 4: [2], 5: [2, 4], 6: [2, 3], 7: [2, 3, 4]}


def _lib():
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd import _native as N

    return N, N.load()


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _masks(*v):
    return (ctypes.c_int * len(v))(*v)


def test_symbols_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptb_hip.h")).read(), flags=re.S)
    N, lib = _lib()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), f"{name} is not declared in include/ptb_hip.h"
        assert hasattr(lib, name) and name in N.SIGNATURES


def _mirror(lib, src=FAKE, dtype=0, dst=FAKE, nviews=2, masks=None, in_is_batch=1, B=1, C=1, D=4, H=4, W=4):
    masks = masks if masks is not None else _masks(0, 7)
    return lib.ptb_volume_mirror(src, dtype, dst, nviews, masks, in_is_batch, B, C, D, H, W, None)


def _reduce(lib, src=FAKE, dtype=0, dst=FAKE, nviews=2, masks=None, op=1, B=1, C=1, D=4, H=4, W=4):
    masks = masks if masks is not None else _masks(0, 7)
    return lib.ptb_volume_mirror_reduce(src, dtype, dst, nviews, masks, op, B, C, D, H, W, None)


def _acc(lib, volume=FAKE, norm=FAKE, weight=FAKE, tiles=FAKE, dtype=0, nviews=2, masks=None, op=1, zs=None, B=1, C=1, d=4):
    masks = masks if masks is not None else _masks(0, 7)
    zs = zs if zs is not None else _i64(0)
    return lib.ptb_volume_mirror_accumulate(volume, norm, weight, tiles, dtype, nviews, masks, op, zs, _i64(0), _i64(0), B, C, d, 4, 4,
                                            8, 8, 8, None)


def _split(lib, volume=FAKE, in_dtype=4, C=1, zs=None, B=1, nviews=2, masks=None, out_dtype=0, out=FAKE):
    masks = masks if masks is not None else _masks(0, 7)
    zs = zs if zs is not None else _i64(0)
    return lib.ptb_volume_split_mirror(volume, in_dtype, 8, 8, 8, C, zs, _i64(0), _i64(0), B, 4, 4, 4, None, None, 0.0, nviews, masks,
                                       out_dtype, out, None)


def _bad_views(call, lib, N):
    assert call(lib, nviews=0) == -1
    assert call(lib, nviews=9, masks=_masks(*range(8), 0)) == -1
    assert call(lib, masks=ctypes.cast(None, N._ip)) == -1
    assert call(lib, masks=_masks(0, 8)) == -1
    assert call(lib, masks=_masks(-1, 0)) == -1


def test_volume_mirror_refuses_bad_arguments():
    N, lib = _lib()
    assert _mirror(lib, src=None) == -1 and _mirror(lib, dst=None) == -1
    _bad_views(_mirror, lib, N)
    assert _mirror(lib, dtype=3) == -1 and _mirror(lib, dtype=-1) == -1
    assert _mirror(lib, in_is_batch=2) == -1
    assert _mirror(lib, B=-1) == -1 and _mirror(lib, C=0) == -1 and _mirror(lib, W=0) == -1
    assert _mirror(lib, D=2048, H=2048, W=2048) == -2         # one plane beyond 32-bit unit indices
    assert _mirror(lib, B=0) == 0                             # nothing to do: returns before any launch


def test_volume_mirror_reduce_refuses_bad_arguments():
    N, lib = _lib()
    assert _reduce(lib, src=None) == -1 and _reduce(lib, dst=None) == -1
    _bad_views(_reduce, lib, N)
    assert _reduce(lib, dtype=3) == -1
    assert _reduce(lib, op=7) == -1 and _reduce(lib, op=-1) == -1
    assert _reduce(lib, B=-1) == -1 and _reduce(lib, H=0) == -1
    assert _reduce(lib, B=0) == 0


def test_volume_mirror_accumulate_refuses_bad_arguments():
    N, lib = _lib()
    assert _acc(lib, volume=None) == -1 and _acc(lib, norm=None) == -1 and _acc(lib, weight=None) == -1 and _acc(lib, tiles=None) == -1
    assert _acc(lib, zs=ctypes.cast(None, N._i64p)) == -1
    _bad_views(_acc, lib, N)
    assert _acc(lib, dtype=3) == -1
    assert _acc(lib, op=7) == -1
    assert _acc(lib, B=-1) == -1 and _acc(lib, C=0) == -1 and _acc(lib, d=0) == -1
    assert _acc(lib, zs=_i64(5)) == -4 and _acc(lib, zs=_i64(-1)) == -4      # roi leaves the accumulator
    assert _acc(lib, B=0) == 0


def test_volume_split_mirror_refuses_bad_arguments():
    N, lib = _lib()
    assert _split(lib, volume=None) == -1 and _split(lib, out=None) == -1
    _bad_views(_split, lib, N)
    assert _split(lib, in_dtype=6) == -1 and _split(lib, out_dtype=3) == -1
    assert _split(lib, C=17) == -2
    assert _split(lib, zs=_i64(1 << 31)) == -4
    assert _split(lib, B=0) == 0
    # ptb_volume_split keeps its own checks (a NULL view list cannot reach it)
    assert lib.ptb_volume_split(FAKE, 4, 8, 8, 8, 1, _i64(0), _i64(0), _i64(0), 0, 4, 4, 4, None, None, 0.0, 0, FAKE, None) == 0
    assert lib.ptb_volume_split(FAKE, 6, 8, 8, 8, 1, _i64(0), _i64(0), _i64(0), 1, 4, 4, 4, None, None, 0.0, 0, FAKE, None) == -1


def test_mirror_views_follow_the_definition():
    from pytorch_toolbelt_amd.inference import MIRROR_VIEWS, mirror_volume_augment, mirror_volume_deaugment

    bits = {"d": 4, "h": 2, "w": 1}
    assert set(MIRROR_VIEWS) == {"d", "h", "w", "dh", "dw", "hw", "dhw"}
    for mirror, views in MIRROR_VIEWS.items():
        allowed = sum(bits[a] for a in mirror)
        assert views == tuple(m for m in range(8) if m & ~allowed == 0) and views[0] == 0 and len(views) == 2 ** len(mirror)
    assert MIRROR_VIEWS["dhw"] == tuple(range(8)) and MIRROR_VIEWS["hw"] == (0, 1, 2, 3) and MIRROR_VIEWS["d"] == (0, 4)
    x = torch.zeros((1, 1, 2, 2, 2))
    for bad in ("", "hd", "x", "dhwd", None, 3, "D"):
        with pytest.raises(ValueError):
            mirror_volume_augment(x, bad)
        with pytest.raises(ValueError):
            mirror_volume_deaugment(x, bad)


def test_split_device_mirror_has_no_cpu_fallback():
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumeSlicer

    slicer = VolumeSlicer((10, 12, 14), (4, 6, 8), (2, 3, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        slicer.split_device(torch.zeros((10, 12, 14), dtype=torch.int16), mirror="dhw")


def _torch_views(x, views):
    return [x.flip(FLIPS[m]) if FLIPS[m] else x for m in views]


def test_host_augment_and_deaugment_equal_the_torch_expression():
    from pytorch_toolbelt_amd.inference import MIRROR_VIEWS, mirror_volume_augment, mirror_volume_deaugment

    g = torch.Generator().manual_seed(0)
    x = torch.rand((2, 3, 4, 5, 6), generator=g)
    for mirror, views in MIRROR_VIEWS.items():
        aug = mirror_volume_augment(x, mirror)
        assert torch.equal(aug, torch.cat(_torch_views(x, views)))
        stack = torch.stack([c.flip(FLIPS[m]) if FLIPS[m] else c for c, m in zip(aug.chunk(len(views)), views)])
        assert torch.equal(mirror_volume_deaugment(aug, mirror, None), stack)
        assert torch.equal(mirror_volume_deaugment(aug, mirror, "mean"), stack.mean(0))
        assert torch.equal(mirror_volume_deaugment(aug, mirror, "sum"), stack.sum(0))
        assert torch.equal(mirror_volume_deaugment(aug, mirror, lambda s, dim: s.amax(dim=dim)), stack.amax(0))
        torch.testing.assert_close(mirror_volume_deaugment(aug, mirror, "gmean"), stack.log().mean(0).exp())
    with pytest.raises(RuntimeError, match="must be divisible by 8"):
        mirror_volume_deaugment(torch.zeros((12, 1, 2, 2, 2)), "dhw")
    with pytest.raises(KeyError):
        mirror_volume_deaugment(torch.zeros((8, 1, 2, 2, 2)), "dhw", "median")


@pytest.mark.parametrize("acc", [torch.float32, torch.float64])
def test_host_merger_integrate_batch_deaugment_equals_torch_expression(acc):
    from pytorch_toolbelt_amd.inference import MIRROR_VIEWS
    from pytorch_toolbelt_amd.inference.tiles_3d import HostBackedVolumeMerger, VolumeMerger, VolumeSlicer

    C = 2
    slicer = VolumeSlicer((11, 9, 13), (6, 4, 8), (3, 2, 5))
    tile = tuple(int(s) for s in slicer.tile_size)
    g = torch.Generator().manual_seed(5)
    n = len(slicer.crops)
    for mirror in ("dhw", "hw", "d"):
        views = MIRROR_VIEWS[mirror]
        V = len(views)
        fused = VolumeMerger(slicer.target_shape, C, slicer.weight, device="cpu", dtype=acc)
        plain = VolumeMerger(slicer.target_shape, C, slicer.weight, device="cpu", dtype=acc)
        assert isinstance(fused, HostBackedVolumeMerger)
        for reduction, red in (("mean", lambda s: s.mean(0)), ("sum", lambda s: s.sum(0)), ("log1p", lambda s: torch.exp(torch.log1p(s).mean(0)) - 1)):
            for b0 in range(0, n, 4):
                rois = slicer.crops[b0:b0 + 4]
                tiles = torch.rand((len(rois), C) + tile, generator=g)
                batch = torch.cat(_torch_views(tiles, views))           # model(mirror_volume_augment(tiles)) for an identity model
                fused.integrate_batch_deaugment(batch, rois, mirror=mirror, reduction=reduction)
                stack = torch.stack([c.flip(FLIPS[m]) if FLIPS[m] else c for c, m in zip(batch.chunk(V), views)])
                plain.integrate_batch(red(stack), rois)
        assert torch.equal(fused.volume, plain.volume) and torch.equal(fused.norm_mask, plain.norm_mask)
        with pytest.raises(ValueError, match="coordinates x views"):
            fused.integrate_batch_deaugment(torch.zeros((V * 2 + 1, C) + tile), slicer.crops[:2], mirror=mirror)
        for reduction in (None, lambda s, dim: s.mean(dim)):
            with pytest.raises(ValueError, match="cannot be fused"):
                fused.integrate_batch_deaugment(torch.zeros((V, C) + tile), slicer.crops[:1], mirror=mirror, reduction=reduction)
    with pytest.raises(ValueError):
        fused.integrate_batch_deaugment(torch.zeros((2, C) + tile), slicer.crops[:1], mirror="z")
