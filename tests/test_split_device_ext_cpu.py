"""CPU: ptb_split_tiles (ImageSlicer.split_device for 16-bit images, OpenCV borders and fp16 / bf16 batches) is declared and exported,
refuses bad arguments before any launch, names OpenCV's border codes, and split_device still refuses host tensors.  Also pins the
per-axis index maps the kernel's borders use to np.pad's results, for pads much wider than the image."""
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


def _header():
    return open(os.path.join(ROOT, "include", "ptb_hip.h")).read()


def test_symbol_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    N, lib = _lib()
    assert re.search(r"\bptb_split_tiles\s*\(", text), "ptb_split_tiles is not declared in include/ptb_hip.h"
    assert hasattr(lib, "ptb_split_tiles") and "ptb_split_tiles" in N.SIGNATURES
    assert hasattr(lib, "ptb_split_tiles_u8") and "ptb_split_tiles_u8" in N.SIGNATURES


def test_border_codes_are_opencvs():
    # cv2.BORDER_CONSTANT = 0, BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_WRAP = 3, BORDER_REFLECT_101 = 4 (OpenCV's core.hpp)
    opencv = {"CONSTANT": 0, "REPLICATE": 1, "REFLECT": 2, "WRAP": 3, "REFLECT_101": 4}
    defined = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define PTB_BORDER_(\w+)\s+(\d+)", _header())}
    assert defined == opencv
    from pytorch_toolbelt_amd import _native as N
    from pytorch_toolbelt_amd.inference import tiles

    for name, v in opencv.items():
        assert getattr(N, f"BORDER_{name}") == v
    assert tiles.BORDER_CONSTANT == 0 and set(tiles._NP_PAD_MODE) == {1, 2, 3, 4}


def _split(lib, N, image=FAKE, in_dtype=3, IH=8, IW=8, IC=1, xs=None, ys=None, B=1, th=4, tw=4, views=(0,), scale=None, bias=None,
           border=0, pad=0.0, out_dtype=0, out=FAKE):
    xs = xs if xs is not None else _i64(*([0] * max(B, 1)))
    ys = ys if ys is not None else _i64(*([0] * max(B, 1)))
    v = N.int_array(list(views)) if views is not None else ctypes.cast(None, N._ip)
    return lib.ptb_split_tiles(image, in_dtype, IH, IW, IC, xs, ys, B, th, tw, len(views or ()), v, scale, bias, border, pad,
                               out_dtype, out, None)


def test_split_tiles_refuses_bad_arguments():
    N, lib = _lib()
    f = (ctypes.c_float * 16)(*([1.0] * 16))
    fp = ctypes.cast(f, N._fp)
    nul64 = ctypes.cast(None, N._i64p)
    # null pointers and sizes
    assert _split(lib, N, image=None) == -1
    assert _split(lib, N, out=None) == -1
    assert _split(lib, N, xs=nul64) == -1 and _split(lib, N, ys=nul64) == -1
    assert _split(lib, N, views=None) == -1
    assert _split(lib, N, IH=0) == -1 and _split(lib, N, IW=0) == -1 and _split(lib, N, IC=0) == -1
    assert _split(lib, N, th=0) == -1 and _split(lib, N, B=-1) == -1
    # element types: float images are refused as unsupported, unknown codes as invalid
    for code in (N.F32, N.F16, N.BF16):
        assert _split(lib, N, in_dtype=code) == -2
    assert _split(lib, N, in_dtype=6) == -1 and _split(lib, N, in_dtype=-1) == -1
    assert _split(lib, N, out_dtype=3) == -1 and _split(lib, N, out_dtype=-1) == -1
    # borders: TRANSPARENT / ISOLATED are OpenCV codes the host split refuses too; anything else is not a border
    assert _split(lib, N, border=5) == -2 and _split(lib, N, border=16) == -2
    assert _split(lib, N, border=6) == -1 and _split(lib, N, border=-1) == -1
    # the constant border value must be a value of the image's type
    assert _split(lib, N, pad=256.0) == -1 and _split(lib, N, pad=-1.0) == -1 and _split(lib, N, pad=0.5) == -1
    assert _split(lib, N, in_dtype=N.U16, pad=65536.0) == -1 and _split(lib, N, in_dtype=N.I16, pad=-32769.0) == -1
    assert _split(lib, N, in_dtype=N.I16, pad=float("nan")) == -1
    # channels, views, affine
    assert _split(lib, N, IC=17) == -2
    assert _split(lib, N, views=tuple(range(8)) + (0,)) == -1          # V > 8
    assert _split(lib, N, views=(8,)) == -1
    assert _split(lib, N, th=4, tw=8, views=(0, 1)) == -1              # a transposing view needs square tiles
    assert _split(lib, N, scale=fp) == -1 and _split(lib, N, bias=fp) == -1
    # tile origins must be addressable with 32-bit coordinates
    assert _split(lib, N, xs=_i64(1 << 31)) == -4 and _split(lib, N, ys=_i64(-(1 << 31))) == -4
    # nothing to do: returns before any launch, for every accepted combination of types and borders
    for in_dtype in (N.U8, N.U16, N.I16):
        for out_dtype in (N.F32, N.F16, N.BF16):
            for border in range(5):
                assert _split(lib, N, in_dtype=in_dtype, out_dtype=out_dtype, border=border, B=0) == 0
    # the constant's range is the image type's; other borders ignore it
    assert _split(lib, N, in_dtype=N.U16, pad=65535.0, B=0) == 0 and _split(lib, N, in_dtype=N.I16, pad=-32768.0, B=0) == 0
    assert _split(lib, N, border=4, pad=-7.5, B=0) == 0


def test_split_tiles_u8_keeps_its_contract():
    N, lib = _lib()

    def u8(image=FAKE, IC=1, B=1, pad=0, out=FAKE):
        return lib.ptb_split_tiles_u8(image, 8, 8, IC, _i64(0), _i64(0), B, 4, 4, 1, N.int_array([0]), None, None, pad, out, None)

    assert u8(image=None) == -1 and u8(out=None) == -1
    assert u8(IC=17) == -2 and u8(IC=17, pad=300) == -2        # the checks keep their order
    assert u8(pad=256) == -1 and u8(pad=-1) == -1
    assert u8(B=0) == 0 and u8(B=0, pad=255) == 0


def test_split_device_refuses_host_tensors():
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer

    s = ImageSlicer((64, 48), 32, 16)
    for dtype in (torch.uint8, torch.int16, torch.uint16):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            s.split_device(torch.zeros((64, 48), dtype=dtype), border_type=4, dtype=torch.bfloat16)


def _index_map(i, n, mode):
    """The per-axis index maps of ptb_edges.hip's border_index (C semantics of % on negative numbers emulated)."""
    if mode == "edge":
        return min(max(i, 0), n - 1)
    if mode == "wrap":
        return i % n
    if mode == "symmetric":
        j = i % (2 * n)
        return j if j < n else 2 * n - 1 - j
    if n == 1:
        return 0
    j = i % (2 * (n - 1))
    return j if j < n else 2 * (n - 1) - j


@pytest.mark.parametrize("mode", ["edge", "wrap", "symmetric", "reflect"])
def test_border_index_maps_equal_np_pad(mode):
    for n in range(1, 9):
        src = np.arange(n)
        for before in range(0, 28, 3):
            for after in (0, 1, 5, 27):
                want = np.pad(src, (before, after), mode=mode)
                got = [src[_index_map(i, n, mode)] for i in range(-before, n + after)]
                assert list(want) == got, (n, before, after)
