"""GPU: VolumeSlicer.split_device and VolumeMerger.merge_crop bit for bit against the host expressions they replace, and the whole
3-D loop on the device (split_device -> model -> integrate_batch -> merge_crop) against the host loop."""
import numpy as np
import pytest
import torch

from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.inference.tiles_3d import HostBackedVolumeMerger, VolumeMerger, VolumeSlicer

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
IN_DTYPES = [torch.uint8, torch.int16, torch.uint16, torch.float16, torch.bfloat16, torch.float32]


def _volume(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == torch.uint8:
        a = rng.integers(0, 256, shape).astype(np.uint8)
    elif dtype == torch.int16:
        a = rng.integers(-3000, 3000, shape).astype(np.int16)
    elif dtype == torch.uint16:
        a = rng.integers(0, 65536, shape).astype(np.uint16)
    else:
        a = (rng.standard_normal(shape) * 300).astype(np.float32)
        return torch.from_numpy(a).to(dtype)
    return torch.from_numpy(a)


def host_split(slicer, vol, value, indices, scale, bias, dtype):
    """The reference expression: the host split of a numpy copy, channels first, stacked, .float(), affine, .to(dtype)."""
    arr = (vol.float() if vol.dtype == torch.bfloat16 else vol).cpu().numpy()
    t = np.stack([np.moveaxis(x, -1, 0) if x.ndim == 4 else x[None] for x in slicer.split(arr, value)])
    if indices is not None:
        t = t[indices]
    r = torch.from_numpy(np.ascontiguousarray(t)).float()
    if scale is not None:
        C = r.shape[1]
        r = r * torch.tensor(scale, dtype=torch.float32).view(1, C, 1, 1, 1) + torch.tensor(bias, dtype=torch.float32).view(1, C, 1, 1, 1)
    return r.to(dtype)


# (volume (D, H, W), tile, step): every geometry pads before and after on every axis, so tiles overhang all six faces
GEOMETRIES = [
    ((19, 23, 29), (8, 12, 16), (5, 7, 9)),        # w = 16: 16-byte stores for every output dtype
    ((11, 10, 13), (6, 8, 12), (4, 5, 7)),         # w = 12: vector fp32, scalar half outputs
    ((12, 11, 10), (5, 6, 13), (3, 4, 6)),         # w = 13: the scalar path
    ((10, 10, 11), (8, 40, 4), (5, 25, 3)),        # 320 rows per tile: several row chunks of 256 rows
]


@pytest.mark.parametrize("in_dtype", IN_DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("C", [1, 3, 16])
def test_split_device_matches_host_split(in_dtype, C):
    for gi, (shape, tile, step) in enumerate(GEOMETRIES):
        slicer = VolumeSlicer(shape, tile, step)
        assert (slicer.pad_before > 0).all() and (slicer.pad_after > 0).all()
        vshape = shape if C == 1 else shape + (C,)
        vol = _volume(vshape, in_dtype, seed=gi * 100 + C)
        dvol = vol.to(DEV)
        rng = np.random.default_rng(gi)
        scale = list(rng.uniform(-2, 2, C).astype(np.float32))
        bias = list(rng.uniform(-100, 100, C).astype(np.float32))
        values = [0, -1024] + ([2.7] if in_dtype.is_floating_point else [])
        for value in values:
            for affine in (False, True):
                for dtype in (torch.float32, torch.float16, torch.bfloat16):
                    sc, bi = (scale, bias) if affine else (None, None)
                    got = slicer.split_device(dvol, scale=sc, bias=bi, value=value, dtype=dtype)
                    want = host_split(slicer, vol, value, None, sc, bi, dtype)
                    assert got.dtype == dtype and got.shape == want.shape
                    assert torch.equal(got.cpu(), want), (shape, tile, value, affine, dtype)


def test_split_device_wide_tiles_and_indices():
    # C = 16 with 264-wide tiles: a row of one tile does not fit the LDS chunk, so a tile is split into column chunks as well
    shape, tile, step = (4, 6, 300), (2, 3, 264), (1, 2, 100)
    slicer = VolumeSlicer(shape, tile, step)
    vol = _volume(shape + (16,), torch.uint16, seed=7)
    dvol = vol.to(DEV)
    for dtype in (torch.float32, torch.bfloat16):
        torch.testing.assert_close(slicer.split_device(dvol, dtype=dtype).cpu(), host_split(slicer, vol, 0, None, None, None, dtype), rtol=0, atol=0)
    odd = VolumeSlicer((4, 6, 300), (2, 3, 261), (1, 2, 100))
    torch.testing.assert_close(odd.split_device(dvol).cpu(), host_split(odd, vol, 0, None, None, None, torch.float32), rtol=0, atol=0)
    n = len(slicer.crops)
    for indices in (slice(1, n, 2), [n - 1, 0, 2], np.array([3]), []):
        got = slicer.split_device(dvol, indices=indices, value=-1024)
        want = host_split(slicer, vol, -1024, indices if not isinstance(indices, list) or indices else None, None, None, torch.float32)
        if isinstance(indices, list) and not indices:
            assert got.shape == (0, 16, 2, 3, 264)
        else:
            assert torch.equal(got.cpu(), want)


def test_split_device_errors():
    slicer = VolumeSlicer((8, 8, 8), (4, 4, 4), (2, 2, 2))
    with pytest.raises(NotImplementedError):
        slicer.split_device(torch.zeros((8, 8, 8), dtype=torch.int32, device=DEV))
    with pytest.raises(NotImplementedError):
        slicer.split_device(torch.zeros((8, 8, 8, 17), dtype=torch.uint8, device=DEV))
    with pytest.raises(NotImplementedError):
        slicer.split_device(torch.zeros((8, 8, 8), dtype=torch.uint8, device=DEV), dtype=torch.float64)
    with pytest.raises(ValueError):
        slicer.split_device(torch.zeros((8, 8, 9), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        slicer.split_device(torch.zeros((8, 8, 8), dtype=torch.uint8, device=DEV), scale=[1.0])
    with pytest.raises(ValueError):
        slicer.split_device(torch.zeros((8, 8, 8), dtype=torch.uint8, device=DEV), bias=[1.0])


def _merger(C, seed, nan=False, skip_last=False, shape=(21, 18, 26), tile=(8, 6, 12), step=(5, 4, 7)):
    slicer = VolumeSlicer(shape, tile, step)
    merger = VolumeMerger(slicer.target_shape, C, slicer.weight, device=DEV)
    g = torch.Generator().manual_seed(seed)
    n = len(slicer.crops)
    # small integers: channels tie often (first maximum must win); quotients are mostly non-integers
    tiles = torch.randint(0, 5, (n, C) + tuple(tile), generator=g).float() * 40
    if nan:
        tiles.view(-1)[torch.randint(0, tiles.numel(), (200,), generator=g)] = float("nan")
    keep = n - 3 if skip_last else n      # uncovered voxels: 0 / 0 = NaN
    merger.integrate_batch(tiles[:keep].to(DEV), slicer.crops[:keep])
    return slicer, merger


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 16])
def test_merge_crop_matches_merge_then_crop(C):
    for nan in (False, True):
        slicer, merger = _merger(C, seed=C, nan=nan, skip_last=nan)
        full = merger.merge()[(slice(None),) + slicer.orignal_image_roi]
        for layout in ("cdhw", "dhwc"):
            moved = full if layout == "cdhw" else full.permute(1, 2, 3, 0)
            kinds = (torch.float32, torch.float16, torch.bfloat16) + (() if nan else (torch.uint8,))
            for dtype in kinds:
                got = merger.merge_crop(slicer, layout=layout, dtype=dtype)
                want = moved.to(dtype)
                assert got.shape == want.shape and got.dtype == dtype
                torch.testing.assert_close(got, want, rtol=0, atol=0, equal_nan=True), (C, nan, layout, dtype)
        for dtype, out in ((torch.uint8, torch.uint8), (torch.int64, torch.int64), (torch.float32, torch.int64)):
            got = merger.merge_crop(slicer, argmax=True, dtype=dtype)
            assert got.dtype == out and torch.equal(got, full.argmax(0).to(out)), (C, nan, dtype)


@pytest.mark.parametrize("C", [2, 3, 4])
def test_merge_crop_windows(C):
    slicer, merger = _merger(C, seed=11)
    full = merger.merge()
    D, H, W = full.shape[1:]
    # unaligned origins, widths that are not multiples of 4, the whole accumulator, a single voxel, an empty window; fp32 "dhwc"
    # with OW % 4 == 0 exchanges its stores through LDS: group counts that are not multiples of 256 (5 * 9 * 3; 23 * 18 * 6 over
    # several workgroups, from an unaligned origin)
    for z0, y0, x0, od, oh, ow in ((1, 2, 3, 5, 7, 9), (0, 0, 0, D, H, W), (D - 1, H - 1, W - 1, 1, 1, 1), (0, 4, 4, 3, 2, 8),
                                   (1, 2, 4, 5, 9, 12), (0, 0, 2, D, H, 24)):
        win = full[:, z0:z0 + od, y0:y0 + oh, x0:x0 + ow]
        for layout in ("cdhw", "dhwc"):
            got = merger.merge_crop((z0, y0, x0, od, oh, ow), layout=layout)
            torch.testing.assert_close(got, win if layout == "cdhw" else win.permute(1, 2, 3, 0), rtol=0, atol=0, equal_nan=True)
        assert torch.equal(merger.merge_crop((z0, y0, x0, od, oh, ow), argmax=True), win.argmax(0))
    assert merger.merge_crop((0, 0, 0, 0, 3, 3)).shape == (C, 0, 3, 3)
    with pytest.raises(ValueError):
        merger.merge_crop((0, 0, 1, D, H, W))


def test_volume_loop_on_device_equals_host_loop():
    """256^3 int16 volume, 96^3 tiles every 48 voxels: split_device -> a fixed elementwise model -> integrate_batch ->
    merge_crop(argmax=True) on the device equals the host loop (slicer.split -> model -> torch-op merger -> crop -> argmax) on every
    voxel."""
    C = 4
    shape, tile, step = (256, 256, 256), 96, 48
    slicer = VolumeSlicer(shape, tile, step)
    vol = _volume(shape, torch.int16, seed=1)
    a = torch.tensor([0.5, -0.25, 1.0, 0.125]).view(1, C, 1, 1, 1)
    b = torch.tensor([10.0, 300.0, -200.0, 50.0]).view(1, C, 1, 1, 1)

    def model(x):           # [B, 1, d, h, w] fp32 -> [B, C, d, h, w]: a product and a sum, each rounded once on either device
        return x * a.to(x.device) + b.to(x.device)

    n, bs = len(slicer.crops), 4
    torch.cuda.synchronize(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    dev_merger = VolumeMerger(slicer.target_shape, C, slicer.weight, device=DEV)
    dvol = vol.to(DEV)
    before = N.calls
    for b0 in range(0, n, bs):
        batch = slicer.split_device(dvol, indices=slice(b0, b0 + bs), value=-1024)
        dev_merger.integrate_batch(model(batch), slicer.crops[b0:b0 + bs])
    labels = dev_merger.merge_crop(slicer, argmax=True, dtype=torch.uint8)
    assert N.calls > before and labels.shape == shape and labels.dtype == torch.uint8
    assert torch.cuda.max_memory_allocated(DEV) - base < 4 * 2 ** 30     # the loop's own device memory

    host = HostBackedVolumeMerger(slicer.target_shape, C, slicer.weight, device="cpu")
    tiles = slicer.split(vol.numpy(), -1024)
    for b0 in range(0, n, bs):
        batch = torch.from_numpy(np.stack(tiles[b0:b0 + bs])[:, None]).float()
        host.integrate_batch(model(batch), slicer.crops[b0:b0 + bs])
    want = host.merge_crop(slicer, argmax=True, dtype=torch.uint8)
    assert torch.equal(labels.cpu(), want)
