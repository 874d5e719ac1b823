"""CPU: the host form of utils.reconstruct -- directional sweeps over ordered keys -- equals the textbook model of tests/reconstruct_cases.py
on every case, bit for bit: reconstruction both ways, regional and h-extrema, hole filling; the fixed one-row example; the documented
divergences from skimage behave as stated; the recipe splits the two discs without a radius; arguments are validated before anything
native loads, and the plan entry point refuses bad shapes without a device."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import ndimage

import nearest_cases as NC
import reconstruct_cases as RC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import (connected_components, distance_transform, fill_holes, h_maxima, h_minima, reconstruction, regional_maxima, regional_minima,
                                        watershed)


def call(case, connectivity, place=torch.from_numpy, **kw):
    """the public call of a case; ``place`` puts an array on a device"""
    dom = None if case.domain is None else place(case.domain)
    kw = dict(connectivity=connectivity, domain=dom, dims=case.dims, **kw)
    img = place(case.image)
    if case.op == "reconstruction":
        return reconstruction(place(case.seed), img, method="erosion" if case.mirror else "dilation", **kw)
    if case.op == "regional":
        return (regional_minima if case.mirror else regional_maxima)(img, **kw)
    if case.op == "h":
        return (h_minima if case.mirror else h_maxima)(img, case.h, **kw)
    return fill_holes(img, **kw)


@pytest.mark.parametrize("name,connectivity", RC.PAIRS)
def test_host_form_equals_the_model(name, connectivity):
    case = RC.CASES[name]
    before = N.calls
    got, sweeps = call(case, connectivity, return_sweeps=True)
    assert N.calls == before, "a CPU tensor reached the native library"
    assert sweeps == (0, 0) and got.shape == case.image.shape
    assert RC.same_bits(got.numpy(), case.expected(connectivity)), name
    assert torch.equal(call(case, connectivity), got) or np.isnan(case.image.astype(np.float32)).any()


def test_the_cases_cover_what_they_claim():
    for h, want in RC.H_ROW_RESULTS.items():
        assert RC.CASES[f"row/h{h}"].expected(4).astype(int).tolist() == [want], h
        assert h_maxima(torch.from_numpy(RC.H_ROW), h, connectivity=4).int().tolist() == [want], h
    assert RC.CASES["constant/maxima"].expected(8).all() and RC.CASES["constant/h_maxima"].expected(4).all()
    c = RC.CASES["clamp/dilation"]
    assert (c.seed > c.image).any() and (c.expected(8) <= c.image).all()
    c = RC.CASES["odd_values/dilation"]
    got = c.expected(8)
    assert np.array_equal(np.isnan(got), np.isnan(c.image)) and not np.signbit(got[got == 0]).any() and (got == 0).sum() > 100
    c = RC.CASES["blobs/fill_domain"]
    lab, n = ndimage.label(c.domain)
    closed = [k for k in range(1, n + 1) if not (lab[0] == k).any() and not (lab[-1] == k).any() and not (lab[:, 0] == k).any() and not (lab[:, -1] == k).any()]
    assert closed and np.isinf(c.expected(4)[lab == closed[0]]).all(), "a domain component that no face reaches holds the highest value"
    c = RC.CASES["serpentine_long/dilation"]
    assert np.array_equal(c.expected(4) == 2.0, np.ones_like(c.domain)) and int(c.domain.sum()) == RC.SERPENTINE_POSITIONS
    for name, least in (("holes0/fill", 20), ("holes_volume/fill", 5)):
        c = RC.CASES[name]
        assert (c.expected(RC.CONNECTIVITIES[c.dims][0]) != c.image).sum() >= least, name


@pytest.mark.parametrize("name", ("holes0/fill", "holes1/fill", "holes_u8/fill", "holes_volume/fill", "holes_volume_stack/fill"))
def test_fill_holes_equals_scipy_on_masks(name):
    case = RC.CASES[name]
    for k, connectivity in enumerate(RC.CONNECTIVITIES[case.dims]):
        want = np.stack([ndimage.binary_fill_holes(e, structure=ndimage.generate_binary_structure(case.dims, case.dims if k else 1)) for e in case.entries(case.image)])
        got = fill_holes(torch.from_numpy(case.image), connectivity=connectivity, dims=case.dims)
        assert got.dtype == torch.from_numpy(case.image).dtype and np.array_equal(got.numpy().astype(bool), want.reshape(case.image.shape)), (name, connectivity)
    first = fill_holes(torch.from_numpy(case.image), dims=case.dims)               # the default: the minimal neighbourhood, scipy's default structure
    assert torch.equal(first, fill_holes(torch.from_numpy(case.image), connectivity=RC.CONNECTIVITIES[case.dims][0], dims=case.dims))


def test_documented_divergences_from_skimage():
    flat = torch.full((5, 6), 3.0)
    assert regional_maxima(flat).all() and regional_minima(flat).all(), "a constant entry is one maximum (skimage: none)"
    seed = torch.tensor([[9.0, 0.0, 0.0, 0.0]])
    mask = torch.tensor([[2.0, 2.0, 1.0, 3.0]])
    assert reconstruction(seed, mask).tolist() == [[2.0, 2.0, 1.0, 1.0]], "seed > mask is clamped (skimage raises)"
    assert reconstruction(-seed, -mask, method="erosion").tolist() == [[-2.0, -2.0, -1.0, -1.0]]
    row = torch.from_numpy(RC.H_ROW)
    assert h_maxima(row, 1.0, connectivity=4).int().tolist() == [RC.H_ROW_RESULTS[1.0]], "dynamic == h is not kept: strictly greater (a residue threshold can differ)"
    assert h_minima(-row, 1.0, connectivity=4).int().tolist() == [RC.H_ROW_RESULTS[1.0]]
    assert torch.equal(h_maxima(row, 0, connectivity=4), regional_maxima(row, connectivity=4))
    assert torch.equal(regional_maxima(torch.tensor([[-0.0, 0.0, -0.0]])), torch.ones((1, 3), dtype=torch.bool)), "-0 and +0 are one plateau"
    out = reconstruction(torch.tensor([[-0.0, -0.0]]), torch.tensor([[-0.0, 5.0]]))
    assert not np.signbit(out.numpy()).any(), "-0 comes back as +0"
    nan = float("nan")
    got = reconstruction(torch.tensor([[nan, 1.0, 4.0]]), torch.tensor([[3.0, nan, 5.0]]))
    assert got.tolist()[0][0] == -np.inf and np.isnan(got.tolist()[0][1]) and got.tolist()[0][2] == 4.0, "a NaN seed is the lowest value; a NaN mask is outside the domain and cuts the path"
    # only the array border is open: a ring of domain closes its inside although the inside touches the outside of the domain
    img = torch.zeros((7, 7), dtype=torch.bool)
    dom = torch.ones((7, 7), dtype=torch.bool)
    dom[2:5, 2:5] = False
    dom[3, 3] = True
    assert bool(fill_holes(img, domain=dom)[3, 3]) and not fill_holes(img, domain=dom)[0, 0]


@pytest.mark.parametrize("connectivity", (4, 8))
def test_two_disc_split_without_a_radius(connectivity):
    """the recipe of the module docstring on two overlapping discs: one component becomes two instances"""
    sem, truth = NC.two_discs()
    t = torch.from_numpy(sem)
    d = distance_transform(t)
    cores, n = connected_components(h_maxima(d, 2.0, domain=t != 0))
    assert int(n) == 2
    inst = watershed(-d, cores, mask=t != 0, connectivity=connectivity)
    assert torch.equal(inst != 0, t != 0) and sorted(np.unique(inst.numpy())) == [0, 1, 2]


def test_dtypes_and_out():
    case = RC.CASES["wide/h_maxima"]
    img = torch.from_numpy(np.round(case.image * 40).astype(np.int16))                 # values every type holds exactly
    want = h_maxima(img.float(), 4.0)
    ref = reconstruction(img.float() - 4, img.float())
    filled = fill_holes(img.float())
    for dtype in (torch.float16, torch.bfloat16, torch.int16):
        assert torch.equal(h_maxima(img.to(dtype), 4.0), want), dtype
        assert torch.equal(reconstruction((img - 4).to(dtype), img.to(dtype)), ref.to(dtype)), dtype
        assert torch.equal(fill_holes(img.to(dtype)), filled.to(dtype)), dtype
    u8 = (img + 100).to(torch.uint8)
    assert torch.equal(h_maxima(u8, 4.0), want) and torch.equal(fill_holes(u8), (filled + 100).to(torch.uint8))
    out = torch.empty(img.shape, dtype=torch.bool)
    assert h_maxima(img, 4.0, out=out) is out and torch.equal(out, want)
    own = img.float()
    assert fill_holes(own, out=own) is own and torch.equal(own, filled)
    assert torch.equal(regional_maxima(img.t()), regional_maxima(img.t().contiguous())) and torch.equal(regional_maxima(img.t()), regional_maxima(img).t())


def test_argument_errors():
    x = torch.zeros((4, 5))
    with pytest.raises(TypeError, match="image must be a tensor"):
        regional_maxima(np.zeros((4, 5), np.float32))
    with pytest.raises(TypeError, match="seed must be a tensor"):
        reconstruction(np.zeros((4, 5), np.float32), x)
    with pytest.raises(TypeError, match="mask must be a tensor"):
        reconstruction(x, None)
    for bad in (torch.float64, torch.int32, torch.int64, torch.bool):
        with pytest.raises(TypeError, match=r"\.float\(\)"):
            h_maxima(x.to(bad), 1.0)
    with pytest.raises(TypeError, match=r"\.float\(\)"):
        fill_holes(x.to(torch.int32))
    assert fill_holes(x.to(torch.bool)).dtype == torch.bool
    with pytest.raises(TypeError, match="same dtype"):
        reconstruction(x.half(), x)
    with pytest.raises(ValueError, match="seed must have shape"):
        reconstruction(torch.zeros((5, 4)), x)
    with pytest.raises(ValueError, match="seed must have shape"):
        reconstruction(torch.zeros((4, 5), device="meta"), x)
    with pytest.raises(ValueError, match="method must be"):
        reconstruction(x, x, method="opening")
    with pytest.raises(ValueError, match="dims must be 2 or 3"):
        regional_maxima(x, dims=4)
    with pytest.raises(ValueError, match=r"\[\*stack, D, H, W\]"):
        regional_maxima(x, dims=3)
    for dims, bad in ((2, 6), (2, True), (3, 8), (2, 26), (2, 0)):
        with pytest.raises(ValueError, match="connectivity must be"):
            regional_minima(x[None], dims=dims, connectivity=bad)
    with pytest.raises(TypeError, match="domain must be bool or uint8"):
        fill_holes(x, domain=torch.ones((4, 5), dtype=torch.int32))
    with pytest.raises(TypeError, match="domain must be a tensor"):
        fill_holes(x, domain=np.ones((4, 5), bool))
    with pytest.raises(ValueError, match="domain must have shape"):
        fill_holes(x, domain=torch.ones((5, 4), dtype=torch.bool))
    for bad in (None, "1", True):
        with pytest.raises(TypeError, match="h must be a number"):
            h_maxima(x, bad)
    for bad in (-1.0, float("inf"), float("nan"), 1e39):
        with pytest.raises(ValueError, match="h must be finite"):
            h_minima(x, bad)
    for bad in (0, -3, 1 << 31):
        with pytest.raises(ValueError, match="max_sweeps"):
            regional_maxima(x, max_sweeps=bad)
    with pytest.raises(TypeError, match="max_sweeps"):
        regional_maxima(x, max_sweeps=2.0)
    for out in (torch.zeros((4, 5)), torch.zeros((5, 4), dtype=torch.bool), torch.zeros((4, 5), dtype=torch.bool, device="meta")):
        with pytest.raises(ValueError, match="out must be"):
            regional_maxima(x, out=out)
    with pytest.raises(ValueError, match="out must be"):
        fill_holes(x, out=torch.zeros((4, 5), dtype=torch.bool))
    with pytest.raises(TypeError, match="out must be"):
        fill_holes(x, out=np.zeros((4, 5), np.float32))
    one = torch.zeros(1, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"2\^31 - 2"):
        fill_holes(one.expand(1 << 16, 1 << 15))


def test_empty_inputs():
    before = N.calls
    got, sweeps = h_maxima(torch.zeros((3, 0, 5)), 1.0, return_sweeps=True)
    assert got.shape == (3, 0, 5) and got.dtype == torch.bool and sweeps == (0, 0)
    assert fill_holes(torch.zeros((0, 2, 2), dtype=torch.uint8), dims=3).dtype == torch.uint8
    out = torch.zeros((2, 0), dtype=torch.int16)
    assert reconstruction(out.clone(), out.clone(), out=out) is out
    assert N.calls == before


# ---------------------------------------------------------------------------------------------------------------- native, host only
VALUES, EXTREMA, H_EXTREMA, FILL = range(4)


def _plan(lib, dims, B, D, H, W, op=0):
    nbytes = ctypes.c_int64(-1)
    return lib.ptb_reconstruct_plan(dims, B, D, H, W, op, ctypes.byref(nbytes)), nbytes.value


def _up16(v):
    return (v + 15) // 16 * 16


def test_plan_workspace_over_a_sweep_of_extents():
    """8 bytes per position (mask key, R), 12 per tile (start flag, two sweep flags), 16 of sweep words"""
    lib = N.load()
    for dims, B, D, H, W in [(2, 1, 1, 1, 1), (2, 3, 1, 17, 65), (2, 1, 1, 5000, 5000), (2, 64, 1, 512, 512), (2, 5_000_000, 1, 1, 1), (2, 1, 1, 64, 64), (2, 1, 1, 65, 129),
                             (3, 1, 1, 1, 1), (3, 2, 5, 9, 33), (3, 1, 256, 256, 256), (3, 4, 9, 17, 23)]:
        n = B * D * H * W
        tiles = B * -(-H // 64) * -(-W // 64) if dims == 2 else B * -(-D // 8) * -(-H // 8) * -(-W // 32)
        for op in range(4):
            rc, nbytes = _plan(lib, dims, B, D, H, W, op)
            assert rc == 0 and nbytes == 16 + 3 * _up16(4 * tiles) + 2 * _up16(4 * n), (dims, B, D, H, W, op)
    assert lib.ptb_reconstruct_plan(2, 1, 1, 4, 4, 0, None) == 0


def test_entry_points_refuse_bad_arguments_without_a_device():
    """The entry points validate before they touch the device, so these calls are safe without a GPU."""
    lib = N.load()
    assert _plan(lib, 4, 1, 1, 4, 4)[0] == -1 and _plan(lib, 2, 1, 2, 4, 4)[0] == -1 and _plan(lib, 2, 0, 1, 4, 4)[0] == -1 and _plan(lib, 3, 1, 4, 0, 4)[0] == -1
    assert _plan(lib, 2, 1, 1, 1 << 16, 1 << 15)[0] == N.PTB_EUNSUPPORTED and _plan(lib, 3, 2, 1 << 10, 1 << 10, 1 << 10)[0] == N.PTB_EUNSUPPORTED
    assert _plan(lib, 2, 1, 1, 4, 4, 4)[0] == -1 and _plan(lib, 2, 1, 1, 4, 4, -1)[0] == -1      # unknown operations
    fake = ctypes.c_void_p(4096)                      # (never dereferenced: every call below is refused first)
    odd = ctypes.c_void_p(4100)
    big = 1 << 40
    inf = float("inf")
    took = (ctypes.c_int * 2)(5, 5)

    def rc(seed=None, mask=fake, dt=N.F32, domain=None, dims=2, B=1, D=1, H=4, W=4, conn=8, op=EXTREMA, erosion=0, h=0.0, top=inf, max_sweeps=100, out=ctypes.c_void_p(8192),
           sweeps=took, work=fake, nbytes=big):
        return lib.ptb_reconstruct(seed, mask, dt, domain, dims, B, D, H, W, conn, op, erosion, h, top, max_sweeps, out, sweeps, work, nbytes, None)

    assert rc(mask=None) == -1 and rc(out=None) == -1 and rc(work=None) == -1
    assert list(took) == [-1, -1]
    assert rc(dt=N.U16) == -1 and rc(dt=-1) == -1 and rc(dt=6) == -1               # element types
    assert rc(dims=1) == -1 and rc(dims=2, D=2) == -1 and rc(H=0) == -1             # dims, extents
    assert rc(conn=6) == -1 and rc(conn=0) == -1 and rc(dims=3, D=2, conn=8) == -1 and rc(dims=3, D=2, conn=4) == -1
    assert rc(op=4) == -1 and rc(op=-1) == -1
    assert rc(op=VALUES) == -1 and rc(op=EXTREMA, seed=fake) == -1                  # a seed exactly where the operation has one
    assert rc(erosion=2) == -1 and rc(op=FILL, erosion=0) == -1
    assert rc(h=1.0) == -1 and rc(op=H_EXTREMA, h=-1.0) == -1 and rc(op=H_EXTREMA, h=inf) == -1 and rc(op=H_EXTREMA, h=float("nan")) == -1
    assert rc(top=1.0) == -1 and rc(op=FILL, erosion=1, top=float("nan")) == -1
    assert rc(max_sweeps=0) == -1 and rc(max_sweeps=-1) == -1
    assert rc(H=1 << 16, W=1 << 15) == N.PTB_EUNSUPPORTED
    need = _plan(lib, 2, 1, 1, 4, 4)[1]
    assert rc(nbytes=need - 1) == -1 and rc(work=odd) == -1 and rc(out=odd) == -1
    assert rc(op=VALUES, seed=fake, out=fake) == -1                                 # the result may not be written over the seed
