"""CPU: ``resample_volume`` without a GPU -- its host form is the torch expression its docstring gives, bit for bit; the argument
errors; the C entry point is declared, bound and validates its arguments before any device call; and the float32 restatement the GPU
tests measure the kernel with (tests/volume_resample_cases.py) follows the float64 operator model on every case."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import volume_resample_cases as VC
from conftest import ROOT


def _inference():
    from pytorch_toolbelt_amd.inference import tiles_3d

    return tiles_3d


def test_host_resample_volume_is_the_torch_expression():
    for k, dtype in enumerate((torch.uint8, torch.int16, torch.uint16)):
        v = VC.volume(dtype, (5, 6, 7, 3), k)
        for out in (torch.float32, torch.float16, torch.bfloat16):
            want = F.interpolate(v.float().permute(3, 0, 1, 2)[None], size=(8, 4, 11), mode="trilinear", align_corners=False)[0]
            got = _inference().resample_volume(v, (8, 4, 11), dtype=out)
            assert got.shape == (8, 4, 11, 3) and got.is_contiguous() and torch.equal(got, want.permute(1, 2, 3, 0).to(out))
    for k, dtype in enumerate((torch.float16, torch.bfloat16, torch.float32)):
        v = VC.volume(dtype, (4, 9, 5), 10 + k)
        want = F.interpolate(v.float()[None, None], size=(9, 3, 5), mode="trilinear", align_corners=True)[0, 0]
        got = _inference().resample_volume(v, (9, 3, 5), align_corners=True)
        assert got.shape == (9, 3, 5) and got.dtype == torch.float32 and torch.equal(got, want)


def test_argument_errors():
    T = _inference()
    for bad in ((4, 4), (4, 4, 0), (4, 4, -1), (4.0, 4, 4), 8, "abc", (True, 2, 2)):
        with pytest.raises(ValueError, match="three positive ints"):
            T.resample_volume(torch.zeros((4, 4, 4)), bad)
    with pytest.raises(NotImplementedError):
        T.resample_volume(torch.zeros((4, 4, 4), dtype=torch.float64), (2, 2, 2))
    with pytest.raises(NotImplementedError):
        T.resample_volume(torch.zeros((4, 4, 4)), (2, 2, 2), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="16 channels"):
        T.resample_volume(torch.zeros((2, 2, 2, 17)), (2, 2, 2))
    with pytest.raises(ValueError):
        T.resample_volume(torch.zeros((4, 4)), (2, 2, 2))


def test_symbol_is_declared_bound_and_exported():
    from pytorch_toolbelt_amd import _native as N

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptb_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint ptb_volume_resize_trilinear\s*\(", header)
    assert len(N.SIGNATURES["ptb_volume_resize_trilinear"][1]) == 13 and hasattr(N.load(), "ptb_volume_resize_trilinear")
    from pytorch_toolbelt_amd import inference

    assert inference.resample_volume is _inference().resample_volume and "resample_volume" in _inference().__all__
    text = open(os.path.join(ROOT, "compat", "pytorch_toolbelt", "inference", "tiles_3d.py")).read()
    assert "from pytorch_toolbelt_amd.inference.tiles_3d import *" in text


def test_argument_validation_without_gpu():
    """The entry point validates every argument before touching the device (tests/test_abi.py::test_argument_validation_without_gpu)."""
    from pytorch_toolbelt_amd import _native as N

    lib = N.load()
    EINVAL, EUNSUPPORTED = -1, -2
    p = 4096      # never dereferenced: every call below returns before a launch

    def resize(vol=p, in_dtype=N.I16, shape=(4, 4, 4), C=1, size=(6, 6, 6), ac=0, out_dtype=N.F32, out=p):
        return lib.ptb_volume_resize_trilinear(vol, in_dtype, *shape, C, *size, ac, out_dtype, out, None)

    assert resize(vol=None) == EINVAL and resize(out=None) == EINVAL
    assert resize(shape=(4, 4, 0)) == EINVAL and resize(C=0) == EINVAL and resize(size=(6, 0, 6)) == EINVAL
    assert resize(in_dtype=6) == EINVAL and resize(in_dtype=-1) == EINVAL and resize(out_dtype=3) == EINVAL
    assert resize(C=17) == EUNSUPPORTED


@pytest.mark.parametrize("ac", (False, True), ids=("half-pixel", "align-corners"))
def test_restatement_follows_the_model(ac):
    """The float32 restatement against the float64 operator on every case of the GPU tests, N(0, 2) values: d <= 2e-6, so that a wrong
    tap rule in the helper cannot hide in the kernel's 4 d.  Largest d seen: 7.6e-7."""
    worst = 0.0
    for k, (extent, size, _) in enumerate(VC.CASES):
        x = VC.volume(torch.float32, (3,) + extent, 50 + k).numpy()
        _, d, _ = VC.tolerance(x, size, ac)
        print(f"{extent} -> {size} ac={ac}: d = {d:.3g}")
        worst = max(worst, d)
    assert worst <= 2e-6


def test_brick_boundary_cases_sit_on_both_sides():
    for ac in (False, True):
        assert VC.brick_floats(*VC.BRICK_FITS, ac) == VC.BRICK_FLOATS
        assert VC.brick_floats(*VC.BRICK_EXCEEDS, ac) > VC.BRICK_FLOATS
        assert VC.brick_floats(*VC.BRICK_FITS, ac, channels=16) > VC.BRICK_FLOATS      # with 16 channels that case gathers directly too
    src = open(os.path.join(ROOT, "pytorch_toolbelt_amd", "csrc", "ptb_volume_resample.hip")).read()
    assert re.search(r"VR_BRICK = %d;" % VC.BRICK_FLOATS, src)
