"""CPU: the 3-D loop edges -- ptb_volume_split / ptb_volume_merge_crop are declared and exported, refuse bad arguments before any
launch (as does the 2-D ptb_merge_crop, which shares the merge + crop kernels), VolumeSlicer.split_device refuses host tensors, and
HostBackedVolumeMerger.merge_crop equals the reference expressions."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

FAKE = ctypes.c_void_p(256)     # never dereferenced: every call below is refused by the argument checks


def _lib():
    import __graft_entry__ as g

    g.build()
    from pytorch_toolbelt_amd import _native as N

    return N, N.load()


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_symbols_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptb_hip.h")).read(), flags=re.S)
    N, lib = _lib()
    for name in ("ptb_volume_split", "ptb_volume_merge_crop"):
        assert re.search(rf"\b{name}\s*\(", text), f"{name} is not declared in include/ptb_hip.h"
        assert hasattr(lib, name) and name in N.SIGNATURES


def _split(lib, volume=FAKE, in_dtype=4, C=1, zs=None, B=1, scale=None, bias=None, out_dtype=0, out=FAKE, d=4):
    zs = zs if zs is not None else _i64(0)
    return lib.ptb_volume_split(volume, in_dtype, 8, 8, 8, C, zs, _i64(0), _i64(0), B, d, 4, 4, scale, bias, 0.0, out_dtype, out, None)


def test_volume_split_refuses_bad_arguments():
    N, lib = _lib()
    f = (ctypes.c_float * 16)(*([1.0] * 16))
    fp = ctypes.cast(f, N._fp)
    assert _split(lib, volume=None) == -1
    assert _split(lib, out=None) == -1
    assert _split(lib, zs=ctypes.cast(None, N._i64p)) == -1
    assert _split(lib, d=0) == -1
    assert _split(lib, B=-1) == -1
    assert _split(lib, in_dtype=6) == -1 and _split(lib, in_dtype=-1) == -1
    assert _split(lib, out_dtype=3) == -1
    assert _split(lib, scale=fp) == -1 and _split(lib, bias=fp) == -1
    assert _split(lib, C=17) == -2
    assert _split(lib, C=0) == -1
    assert _split(lib, zs=_i64(1 << 31)) == -4
    assert _split(lib, B=0) == 0              # nothing to do: returns before any launch


def _crop(lib, vol=FAKE, norm=FAKE, C=2, window=(0, 0, 0, 4, 4, 4), layout=0, kind=0, out=FAKE):
    return lib.ptb_volume_merge_crop(vol, norm, C, 8, 8, 8, *window, layout, kind, out, None)


def test_volume_merge_crop_refuses_bad_arguments():
    N, lib = _lib()
    assert _crop(lib, vol=None) == -1 and _crop(lib, norm=None) == -1 and _crop(lib, out=None) == -1
    assert _crop(lib, C=0) == -1
    assert _crop(lib, layout=2) == -1
    assert _crop(lib, kind=6) == -1 and _crop(lib, kind=-1) == -1
    assert _crop(lib, window=(5, 0, 0, 4, 4, 4)) == -4
    assert _crop(lib, window=(0, -1, 0, 4, 4, 4)) == -4
    assert _crop(lib, window=(0, 0, 1, 4, 4, 8)) == -4
    assert _crop(lib, C=300, kind=2) == -2
    assert _crop(lib, window=(0, 0, 0, 0, 4, 4)) == 0     # empty window: nothing to launch


def _crop2(lib, image=FAKE, norm=FAKE, C=2, window=(0, 0, 4, 4), layout=0, kind=0, out=FAKE):
    return lib.ptb_merge_crop(image, norm, C, 8, 8, *window, layout, kind, out, None)


def test_merge_crop_refuses_bad_arguments():
    """ptb_merge_crop (2-D) keeps its own checks and their order: the window is checked before layout and kind, kinds 4 and 5
    (fp16 / bf16 output) are refused, and norm may be NULL."""
    N, lib = _lib()
    assert _crop2(lib, image=None) == -1 and _crop2(lib, out=None) == -1
    assert _crop2(lib, C=0) == -1
    assert _crop2(lib, window=(0, 0, -1, 4)) == -1
    assert _crop2(lib, window=(5, 0, 4, 4)) == -4
    assert _crop2(lib, window=(0, -1, 4, 4)) == -4
    assert _crop2(lib, window=(0, 1, 4, 8)) == -4
    assert _crop2(lib, window=(5, 0, 4, 4), layout=2, kind=6) == -4    # the window first
    assert _crop2(lib, layout=2) == -1 and _crop2(lib, layout=-1) == -1
    for kind in (-1, 4, 5, 6):
        assert _crop2(lib, kind=kind) == -1, kind
        assert _crop2(lib, norm=None, kind=kind) == -1, kind
    assert _crop2(lib, C=300, kind=2) == -2
    assert _crop2(lib, window=(0, 0, 0, 4)) == 0 and _crop2(lib, window=(0, 0, 4, 0)) == 0     # empty window: nothing to launch
    assert _crop2(lib, norm=None, window=(0, 0, 0, 4)) == 0                                   # norm == NULL is accepted


def test_split_device_has_no_cpu_fallback():
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumeSlicer

    slicer = VolumeSlicer((10, 12, 14), (4, 6, 8), (2, 3, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        slicer.split_device(torch.zeros((10, 12, 14), dtype=torch.int16))


def _host_merger(C=3, dtype=torch.float32):
    from pytorch_toolbelt_amd.inference.tiles_3d import HostBackedVolumeMerger, VolumeMerger, VolumeSlicer

    slicer = VolumeSlicer((11, 9, 13), (6, 4, 8), (3, 2, 5))
    merger = VolumeMerger(slicer.target_shape, C, slicer.weight, device="cpu", dtype=dtype)
    assert isinstance(merger, HostBackedVolumeMerger)
    g = torch.Generator().manual_seed(3)
    tiles = torch.randint(0, 4, (len(slicer.crops), C) + tuple(int(s) for s in slicer.tile_size), generator=g).to(dtype) * 50
    merger.integrate_batch(tiles[:-2], slicer.crops[:-2])     # the last tiles stay out: some voxels are never covered (NaN)
    return slicer, merger


@pytest.mark.parametrize("acc", [torch.float32, torch.float64])
def test_host_merge_crop_equals_merge_then_crop(acc):
    slicer, merger = _host_merger(dtype=acc)
    window = (slice(None),) + slicer.orignal_image_roi
    full = merger.merge()[window]
    for layout in ("cdhw", "dhwc"):
        moved = full if layout == "cdhw" else full.permute(1, 2, 3, 0)
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            torch.testing.assert_close(merger.merge_crop(slicer, layout=layout, dtype=dtype), moved.to(dtype), rtol=0, atol=0, equal_nan=True)
    finite = torch.nan_to_num(full, nan=0.0)
    assert torch.isfinite(finite).all()
    for dtype, want in ((torch.uint8, torch.uint8), (torch.int64, torch.int64), (torch.float32, torch.int64)):
        got = merger.merge_crop(slicer, argmax=True, dtype=dtype)
        assert got.dtype == want and torch.equal(got, full.argmax(0).to(want))
    z0, y0, x0 = 1, 2, 3
    explicit = merger.merge_crop((z0, y0, x0, 4, 5, 6), layout="dhwc")
    torch.testing.assert_close(explicit, merger.merge()[:, 1:5, 2:7, 3:9].permute(1, 2, 3, 0).float(), rtol=0, atol=0, equal_nan=True)


def test_host_merge_crop_refuses_bad_windows():
    slicer, merger = _host_merger()
    with pytest.raises(ValueError):
        merger.merge_crop((0, 0, 0, 100, 1, 1))
    with pytest.raises(ValueError):
        merger.merge_crop(slicer, layout="hwc")
    with pytest.raises(NotImplementedError):
        merger.merge_crop(slicer, dtype=torch.int32)
