"""GPU: ImageSlicer.split_device for 16-bit images, the five OpenCV borders and fp16 / bf16 batches (ptb_split_tiles), bit for bit
against the host expression it replaces:

    x = np.stack([moveaxis(t, -1, 0) for t in slicer.split(image, border_type, value)])[indices].astype(float32)
    x = x * scale[c] + bias[c]                      (optional; two fp32 roundings)
    out = image_augment(x, augment) -> torch .to(dtype)

Every step is exact or a single rounding that the kernel performs the same way (8- / 16-bit integers widen exactly, the augment
views only move elements, fp32 -> fp16 / bf16 rounds to nearest even), so the comparisons are on the bits."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import tta_oracle as AO

pytestmark = pytest.mark.gpu

IN_DTYPES = [torch.uint8, torch.uint16, torch.int16]
OUT_DTYPES = [torch.float32, torch.float16, torch.bfloat16]
BORDERS = [0, 1, 2, 3, 4]   # cv2.BORDER_CONSTANT, REPLICATE, REFLECT, WRAP, REFLECT_101
AUGMENTS = [None, "fliplr", "d2", "d4"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def native():
    from pytorch_toolbelt_amd import _native as N

    lib = N.load()
    yield N
    lib.ptb_set_tunable(0, 32)
    lib.ptb_set_tunable(1, 0)


def _image(shape, dtype, seed):
    """Random full-range pixels, with the extremes of the type written into the first pixels (they land in tiles and borders)."""
    rng = np.random.default_rng(seed)
    info = np.iinfo(torch.empty(0, dtype=dtype).numpy().dtype)
    a = rng.integers(int(info.min), int(info.max) + 1, shape).astype(info.dtype)
    flat = a.reshape(-1)
    head = [info.min, info.max, 0, info.max][:flat.size]
    flat[:len(head)] = head
    if flat.size > 4:
        flat[-2:] = [info.max, info.min]
    return a


def _expected(slicer, img, indices, augment, scale, bias, value, border, dtype):
    tiles = slicer.split(img, border, value)
    x = np.stack([t[None] if t.ndim == 2 else np.moveaxis(t, -1, 0) for t in tiles])
    if indices is not None:
        x = x[indices]
    x = x.astype(np.float32)
    if scale is not None:
        s = np.asarray(scale, dtype=np.float32).reshape(1, -1, 1, 1)
        b = np.asarray(bias, dtype=np.float32).reshape(1, -1, 1, 1)
        x = (x * s).astype(np.float32) + b
    if augment is not None:
        x = AO.image_augment(x, augment)
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def _check(got, want):
    got = got.cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape)
    if want.dtype == torch.float32:
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    else:
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def _affine(C, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0007, 0.013, C).astype(np.float32), rng.uniform(-3, 3, C).astype(np.float32)


@pytest.mark.parametrize("out_dtype", OUT_DTYPES, ids=str)
@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("in_dtype", IN_DTYPES, ids=str)
def test_split_device_dtypes_borders_augments(in_dtype, border, out_dtype, dev):
    """in-dtype x border x out-dtype, each with every augment and the affine on / off."""
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer

    img = _image((70, 90, 3), in_dtype, seed=border)
    s = ImageSlicer(img.shape, 32, 16)          # automatic margins: every tile row / column at an edge hangs over the image
    value = {torch.uint8: 7, torch.uint16: -1, torch.int16: -32768}[in_dtype]   # uint16: -1 wraps to 65535 as in np.pad
    dimg = torch.from_numpy(img).to(dev)
    n = len(s.crops)
    scale, bias = _affine(3, border)
    for augment in AUGMENTS:
        for affine in (False, True):
            sc, bi = (scale, bias) if affine else (None, None)
            idx = [n - 1, 0, n // 2, 1]
            got = s.split_device(dimg, idx, augment=augment, scale=sc, bias=bi, value=value, border_type=border, dtype=out_dtype)
            _check(got, _expected(s, img, idx, augment, sc, bi, value, border, out_dtype))
    got = s.split_device(dimg, border_type=border, value=value, dtype=out_dtype)
    _check(got, _expected(s, img, None, None, None, None, value, border, out_dtype))


@pytest.mark.parametrize("C", [None, 3, 4, 13])
@pytest.mark.parametrize("in_dtype", IN_DTYPES, ids=str)
def test_split_device_channels(in_dtype, C, dev):
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer

    shape = (66, 52) if C is None else (66, 52, C)
    img = _image(shape, in_dtype, seed=C or 1)
    s = ImageSlicer(img.shape, 24, 12)
    dimg = torch.from_numpy(img).to(dev)
    scale, bias = _affine(C or 1, 5)
    for border, augment, out_dtype in ((4, "d4", torch.bfloat16), (2, "d2", torch.float16), (0, None, torch.float32), (3, "fliplr", torch.bfloat16)):
        got = s.split_device(dimg, augment=augment, scale=scale, bias=bias, value=9, border_type=border, dtype=out_dtype)
        _check(got, _expected(s, img, None, augment, scale, bias, 9, border, out_dtype))


@pytest.mark.parametrize("chunk_rows", [16, 32, 64])
@pytest.mark.parametrize("shape,tile,step,margin,augment", [
    ((300, 420, 3), (128, 128), (64, 64), 0, "d4"),
    ((257, 190, 4), (64, 96), (32, 48), (5, 9, 3, 20), "d2"),
    ((130, 131), (64, 64), (64, 64), 0, "d4"),
    ((100, 90, 1), (40, 36), (20, 12), 7, "flips"),
    ((90, 75, 3), (36, 36), (18, 18), 0, "d4"),
])
def test_split_device_geometries(shape, tile, step, margin, augment, chunk_rows, dev, native):
    """The geometries of test_split_device_matches_oracle, for each chunk-rows setting (ptb_set_tunable key 0)."""
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer

    native.load().ptb_set_tunable(0, chunk_rows)
    s = ImageSlicer(shape[:2], tile, step, image_margin=margin)
    C = 1 if len(shape) == 2 else shape[2]
    scale, bias = _affine(C, 11)
    n = len(s.crops)
    for k, (in_dtype, border, out_dtype) in enumerate([(torch.uint16, 4, torch.bfloat16), (torch.int16, 1, torch.float32),
                                                       (torch.uint8, 2, torch.float16), (torch.uint16, 3, torch.float32)]):
        img = _image(shape, in_dtype, seed=k)
        dimg = torch.from_numpy(img).to(dev)
        for idx in (None, slice(1, n, 2), [n - 1, 0, n // 2]):
            ids = np.arange(n)[idx] if idx is not None else None
            got = s.split_device(dimg, idx, augment=augment, scale=scale, bias=bias, border_type=border, dtype=out_dtype)
            _check(got, _expected(s, img, ids, augment, scale, bias, 0, border, out_dtype))


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("in_dtype", IN_DTYPES, ids=str)
def test_split_device_margins_wider_than_the_image(in_dtype, border, dev):
    """Tiny images under large tiles: the border's index map folds coordinates many image widths away."""
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer

    for shape, tile, step, margin in (((5, 7, 3), 32, 16, 0), ((5, 7), 32, 32, 40), ((3, 2, 2), (12, 16), (4, 8), (21, 13, 30, 2))):
        img = _image(shape, in_dtype, seed=3)
        s = ImageSlicer(shape[:2], tile, step, image_margin=margin)
        dimg = torch.from_numpy(img).to(dev)
        for augment, out_dtype in ((None, torch.float32), ("fliplr", torch.bfloat16), ("d2", torch.float16)):
            got = s.split_device(dimg, augment=augment, value=1, border_type=border, dtype=out_dtype)
            _check(got, _expected(s, img, None, augment, None, None, 1, border, out_dtype))


@pytest.mark.parametrize("border", BORDERS)
def test_split_device_one_pixel_wide_image(border, dev):
    """n == 1 along an axis: REFLECT_101 has no period there (np.pad repeats the pixel), every border must still agree."""
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer

    for shape in ((40, 1), (1, 37, 3), (1, 1)):
        img = _image(shape, torch.uint16, seed=4)
        s = ImageSlicer(shape[:2], 8, 4)
        dimg = torch.from_numpy(img).to(dev)
        for augment in (None, "d4"):
            got = s.split_device(dimg, augment=augment, value=5, border_type=border, dtype=torch.bfloat16)
            _check(got, _expected(s, img, None, augment, None, None, 5, border, torch.bfloat16))


def test_split_device_more_tiles_than_one_launch_group(dev):
    """> 64 tiles: several launch groups; chunk-major rows must still be k*n + tile, for every border."""
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer

    img = _image((200, 264, 3), torch.uint16, seed=6)
    s = ImageSlicer(img.shape, 32, 16)
    assert len(s.crops) > 128
    dimg = torch.from_numpy(img).to(dev)
    for border, out_dtype in ((4, torch.bfloat16), (3, torch.float32), (0, torch.float16)):
        got = s.split_device(dimg, augment="d4", border_type=border, value=-1, dtype=out_dtype)
        _check(got, _expected(s, img, None, "d4", None, None, -1, border, out_dtype))


@pytest.mark.parametrize("chunk_rows", [16, 32, 64])
@pytest.mark.parametrize("scalar", [0, 1])
def test_split_device_tunables(scalar, chunk_rows, dev, native):
    """Key 1 forces the scalar kernel and key 0 picks the chunk rows, for every new instance (in x out dtype)."""
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer

    lib = native.load()
    lib.ptb_set_tunable(1, scalar)
    lib.ptb_set_tunable(0, chunk_rows)
    s = ImageSlicer((150, 133), 64, 48)
    scale, bias = _affine(4, 8)
    for k, in_dtype in enumerate(IN_DTYPES):
        img = _image((150, 133, 4), in_dtype, seed=k)
        dimg = torch.from_numpy(img).to(dev)
        for out_dtype in OUT_DTYPES:
            border = (k + OUT_DTYPES.index(out_dtype)) % 5
            before = native.calls
            got = s.split_device(dimg, augment="d4", scale=scale, bias=bias, value=2, border_type=border, dtype=out_dtype)
            assert native.calls > before
            _check(got, _expected(s, img, None, "d4", scale, bias, 2, border, out_dtype))


@pytest.mark.parametrize("scalar", [0, 1])
def test_uint8_constant_fp32_through_new_keywords_equals_old_call(scalar, dev, native):
    """The new keywords at their defaults, spelled out, and ptb_split_tiles_u8 itself all give the same bits."""
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer

    N = native
    lib = N.load()
    lib.ptb_set_tunable(1, scalar)
    img = _image((300, 420, 3), torch.uint8, seed=9)
    s = ImageSlicer(img.shape, 128, 64)
    dimg = torch.from_numpy(img).to(dev)
    scale, bias = _affine(3, 9)
    old = s.split_device(dimg, None, "d4", scale, bias, 3)
    new = s.split_device(dimg, None, "d4", scale, bias, 3, border_type=0, dtype=torch.float32)
    assert torch.equal(old.view(torch.int32), new.view(torch.int32))
    raw = torch.full_like(old, float("nan"))
    xy = np.ascontiguousarray(np.asarray(s.bbox_crops, dtype=np.int64)[:, :2].T)
    from pytorch_toolbelt_amd.inference.tta import AUGMENT_VIEWS

    views = list(AUGMENT_VIEWS["d4"])
    sc, bi = np.ascontiguousarray(scale), np.ascontiguousarray(bias)
    rc = lib.ptb_split_tiles_u8(dimg.data_ptr(), 300, 420, 3, xy[0].ctypes.data_as(N._i64p), xy[1].ctypes.data_as(N._i64p), len(s.crops),
                                128, 128, len(views), N.int_array(views), sc.ctypes.data_as(N._fp), bi.ctypes.data_as(N._fp), 3,
                                ctypes.c_void_p(raw.data_ptr()), N.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(raw.view(torch.int32), old.view(torch.int32))
    _check(old, _expected(s, img, None, "d4", scale, bias, 3, 0, torch.float32))


def test_split_device_ext_errors(dev):
    from pytorch_toolbelt_amd.inference.tiles import ImageSlicer

    s = ImageSlicer((64, 48, 3), (32, 16), (16, 16))
    img = torch.zeros((64, 48, 3), dtype=torch.uint16, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.split_device(img.cpu(), border_type=4, dtype=torch.bfloat16)
    for bad in (torch.float32, torch.float16, torch.bfloat16, torch.int32):      # float images stay refused
        with pytest.raises(NotImplementedError):
            s.split_device(torch.zeros((64, 48, 3), dtype=bad, device=dev))
    for bad in (torch.float64, torch.uint8, torch.int16):
        with pytest.raises(NotImplementedError):
            s.split_device(img, dtype=bad)
    for bad in (5, 16, 7, -1):
        with pytest.raises(NotImplementedError):
            s.split_device(img, border_type=bad)
    with pytest.raises(ValueError):
        s.split_device(img[:32], dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        s.split_device(img, augment="d4", border_type=4)       # non-square tiles cannot take transposing views
    with pytest.raises(KeyError):
        s.split_device(img, augment="d8", dtype=torch.float16)
    with pytest.raises(ValueError):
        s.split_device(img, scale=[1, 1, 1], border_type=2)
    with pytest.raises(NotImplementedError):
        s.split_device(torch.zeros((64, 48, 17), dtype=torch.int16, device=dev), border_type=1)   # C > 16
    with pytest.raises(RuntimeError, match="invalid argument"):
        s.split_device(torch.zeros((64, 48, 3), dtype=torch.uint8, device=dev), value=300)                                         # uint8 keeps its 0..255 check
    out = s.split_device(img, [], border_type=3, dtype=torch.bfloat16)
    assert out.shape == (0, 3, 32, 16) and out.dtype == torch.bfloat16
