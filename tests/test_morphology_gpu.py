"""GPU: the walk kernels of csrc/ptb_morphology.hip against scipy.ndimage on the float64-widened input with exact equality, and against the
host form bit for bit: an entry of more than one strip and band with odd remainders, planes smaller than the window, a stack; footprints
that use every level and the full halo, an even one and one with two runs in a row and no origin; both border forms; every dtype; a
base one element into its buffer; out=; run-to-run identity; one native call per public call; the saturating differences."""
import numpy as np
import pytest
import torch

from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import morphology as MO
from test_morphology_cpu import BINARY, GREY, TWO_RUNS, as_array, scipy_binary, scipy_grey

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FOOTPRINTS = {"3": 3, "4x2": (4, 2), "disk31": MO.disk(31), "two_runs": TWO_RUNS}
GREY_SHAPES = {"strips_and_bands": (MO.BAND + 3, MO.STRIP + 5), "1x1": (1, 1), "2x70": (2, 70), "stack": (3, 20, 40)}
BIT_SHAPES = {"strips_and_bands": (MO.BIT_BAND + 3, 32 * MO.BIT_WORDS + 5), "1x1": (1, 1), "2x70": (2, 70), "stack": (3, 20, 40)}


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _offset(t):
    """a contiguous device copy of ``t`` that starts one element into its buffer"""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:].view(t.shape).copy_(t)
    return buf[1:].view(t.shape)


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]) if t.dtype != torch.bool else t


def _call(fn, x, *args, **kw):
    before = N.calls
    got = fn(x, *args, **kw)
    assert N.calls == before + 1, "one native call per public call"
    assert got.shape == x.shape and got.device == x.device
    return got


@pytest.mark.parametrize("border", (None, 3.0))
@pytest.mark.parametrize("fp", FOOTPRINTS)
@pytest.mark.parametrize("shape", GREY_SHAPES)
def test_grey_walk_equals_scipy_and_the_host_form(shape, fp, border):
    x = np.random.default_rng(11).integers(-9, 10, GREY_SHAPES[shape]).astype(np.float32)        # small integers: every difference is exact
    planes = x.reshape((-1,) + x.shape[-2:])
    d = _dev(x)
    want = scipy_grey(planes.astype(np.float64), as_array(FOOTPRINTS[fp]), border)      # once per case, shared by the seven functions
    for op in GREY:
        got = _call(getattr(MO, op), d, FOOTPRINTS[fp], border_value=border)
        assert got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy().astype(np.float64), want[op].reshape(x.shape)), op
        assert torch.equal(_bits(got.cpu()), _bits(getattr(MO, op)(d.cpu(), FOOTPRINTS[fp], border_value=border))), op


@pytest.mark.parametrize("border", (None, 0, 1))
@pytest.mark.parametrize("fp", FOOTPRINTS)
@pytest.mark.parametrize("shape", BIT_SHAPES)
def test_bit_plane_walk_equals_scipy_and_the_host_form(shape, fp, border):
    rng = np.random.default_rng(12)
    m = rng.random(BIT_SHAPES[shape]) < (0.97 if fp == "disk31" else 0.7)       # (dense enough for an erosion by the large disk to leave something)
    planes = m.reshape((-1,) + m.shape[-2:])
    d = _dev(m.astype(np.uint8))
    want = scipy_binary(planes, as_array(FOOTPRINTS[fp]), border)
    for op in BINARY:
        got = _call(getattr(MO, op), d, FOOTPRINTS[fp], border_value=border)
        assert got.dtype == torch.bool
        assert np.array_equal(got.cpu().numpy(), want[op].reshape(m.shape)), op
        assert torch.equal(got.cpu(), getattr(MO, op)(d.cpu(), FOOTPRINTS[fp], border_value=border)), op


@pytest.mark.parametrize("dtype", MO.M.VALUE_CODES, ids=str)
def test_every_grey_dtype_from_an_odd_base_twice(dtype):
    x = np.random.default_rng(13).integers(0, 201, (37, 70))
    d = _offset(_dev(x, dtype))
    for border in (None, 100):
        wants = scipy_grey(x[None].astype(np.float64), as_array((4, 2)), border)
        for op in GREY:
            got = _call(getattr(MO, op), d, (4, 2), border_value=border)
            assert got.dtype == dtype
            want = wants[op][0]
            if op in GREY[4:] and not dtype.is_floating_point:
                want = np.clip(want, 0 if dtype == torch.uint8 else -32768, 255 if dtype == torch.uint8 else 32767)
            assert np.array_equal(got.cpu().to(torch.float64).numpy(), want), (op, border)      # (halves are compared after widening)
            assert torch.equal(_bits(got.cpu()), _bits(getattr(MO, op)(d.cpu(), (4, 2), border_value=border))), (op, border)
            assert torch.equal(_bits(getattr(MO, op)(d, (4, 2), border_value=border)), _bits(got)), "a second run: the same bits"


@pytest.mark.parametrize("dtype", MO.M.ELEM_BYTES, ids=str)
def test_every_label_dtype_and_both_object_rules(dtype):
    """33 x 110 int16 rows are no multiple of 16 bytes: the peeled loads; 16 x 64: the 16-byte ones; and each again from a base one element in"""
    for shape in ((33, 110), (16, 64)):
        classes = np.random.default_rng(14).integers(0, 4, shape)
        for place in (lambda t: t, _offset):
            x = place(_dev(classes != 0) if dtype == torch.bool else _dev(classes, dtype))
            for kw in (dict(), dict(foreground=1), dict(background=3), dict(foreground=1 << 40)):
                if dtype == torch.bool and "background" in kw:
                    continue
                for op in BINARY:
                    assert torch.equal(_call(getattr(MO, op), x, MO.disk(2), **kw).cpu(), getattr(MO, op)(x.cpu(), MO.disk(2), **kw)), (shape, kw, op)


def test_out_direct_misaligned_and_the_input_itself():
    x = _dev(np.random.default_rng(15).integers(0, 255, (45, 50)), torch.uint8)
    want = MO.opening(x.cpu(), MO.disk(2))
    out = torch.zeros_like(x)
    assert _call(MO.opening, x, MO.disk(2), out=out) is out and torch.equal(out.cpu(), want)
    off = _offset(torch.zeros_like(x))
    assert MO.opening(x, MO.disk(2), out=off) is off and torch.equal(off.cpu(), want)
    own = x.clone()
    assert MO.opening(own, MO.disk(2), out=own) is own and torch.equal(own.cpu(), want)
    assert torch.equal(MO.opening(x.t().contiguous().t(), MO.disk(2)).cpu(), want)             # other strides are copied first
    mask = MO.binary_closing(x.cpu(), 3, background=7)
    for dtype in (torch.bool, torch.uint8):
        out = torch.ones(x.shape, dtype=dtype, device=DEV)
        assert _call(MO.binary_closing, x, 3, background=7, out=out) is out and torch.equal(out.cpu().bool(), mask)
    own = x.clone()
    assert MO.binary_closing(own, 3, background=7, out=own) is own and torch.equal(own.cpu().bool(), mask)
    before = N.calls                                                           # empty inputs launch nothing
    assert MO.erosion(torch.zeros((2, 0, 4), device=DEV)).shape == (2, 0, 4) and N.calls == before


def test_differences_saturate_on_uint8_with_a_footprint_that_lacks_the_origin():
    x = np.random.default_rng(16).integers(0, 256, (40, 41)).astype(np.uint8)
    # (an opening never exceeds its input and a closing never falls below it, whatever the footprint: the top-hats go below zero at a border value only)
    for op, border in (("morphological_gradient", None), ("white_tophat", 255), ("black_tophat", 0)):
        exact = scipy_grey(x[None].astype(np.float64), TWO_RUNS, border)[op][0]
        assert exact.min() < 0, "the case holds differences below zero"
        got = _call(getattr(MO, op), _dev(x), TWO_RUNS, border_value=border)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), np.clip(exact, 0, 255).astype(np.uint8)), op
