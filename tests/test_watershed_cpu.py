"""CPU: the host form of utils.watershed -- one priority flood -- equals the two-search model of tests/watershed_cases.py on every case:
labels, pass height and seed, bit for bit; where exactly one marker label attains the pass height the result is that label; a constant
landscape gives the multi-source breadth-first search with smallest-index ties; the documented recipe splits the two discs; arguments
are validated before anything native loads, and the plan entry point refuses bad shapes and flags without a device."""
import ctypes

import numpy as np
import pytest
import torch

import nearest_cases as NC
import watershed_cases as WC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import connected_components, distance_transform, match_instances, watershed


def _tensors(case):
    return torch.from_numpy(case.height), torch.from_numpy(case.markers), None if case.mask is None else torch.from_numpy(case.mask)


@pytest.mark.parametrize("name,connectivity", WC.PAIRS)
def test_host_form_equals_the_model(name, connectivity):
    case = WC.CASES[name]
    labels, cost, seed = case.expected(connectivity)
    h, m, mask = _tensors(case)
    before = N.calls
    got = watershed(h, m, mask=mask, connectivity=connectivity, background=case.background, dims=case.dims, return_cost=True, return_seed=True, return_sweeps=True)
    assert N.calls == before, "a CPU tensor reached the native library"
    assert got[0].dtype == m.dtype and got[0].shape == m.shape and np.array_equal(got[0].numpy(), labels), name
    assert got[1].dtype == torch.float32 and np.array_equal(got[1].numpy().view(np.int32), cost.view(np.int32)), name
    assert got[2].dtype == torch.int32 and np.array_equal(got[2].numpy(), seed), name
    assert got[3] == (0, 0)
    assert torch.equal(watershed(h, m, mask=mask, connectivity=connectivity, background=case.background, dims=case.dims), got[0])
    # the contract's corollaries: background exactly where nothing is reached; a seed holds its own index; nothing outside the flooded set
    reached = seed >= 0
    assert np.array_equal(reached, cost != np.inf) and not reached[~case.flooded].any() and reached[case.seeds].all()
    for s, k in zip(case.entries(seed), case.entries(case.seeds)):
        assert np.array_equal(s.ravel()[k.ravel()], np.flatnonzero(k.ravel())), "a seed names itself"


def test_the_cases_cover_what_they_claim():
    assert not (WC.CASES["stack_hole"].seeds[1]).any() and (WC.CASES["stack_hole"].expected(8)[2][1] == -1).all()
    assert np.isinf(WC.CASES["stack_hole"].expected(8)[1][1]).all() and (WC.CASES["stack_hole"].expected(8)[0][1] == 0).all()
    c = WC.CASES["seeds_outside_mask"]
    assert ((c.markers != 0) & ~c.flooded).any() and (c.expected(8)[0][~c.flooded] == 0).all()
    c = WC.CASES["background_unheld"]
    assert c.seeds[c.flooded].all() and np.array_equal(c.expected(4)[0][c.flooded], c.markers[c.flooded]) and (c.expected(4)[0][~c.flooded] == 300 % 256).all()
    c = WC.CASES["signed_zero"]
    cost = c.expected(4)[1]
    assert not np.signbit(cost[cost == 0]).any() and (cost == 0).sum() > 500, "the zeros of both signs are one plateau"
    for name in ("serpentine_h", "serpentine_v", "serpentine_long", "volume_corridor"):
        c = WC.CASES[name]
        labels, _, seed = c.expected(WC.CONNECTIVITIES[c.dims][0])
        assert np.array_equal(labels != 0, c.mask) and (seed[c.mask] == 0).all(), name


@pytest.mark.parametrize("name", WC.UNAMBIGUOUS_CASES)
def test_unambiguous_positions_take_the_only_label(name):
    case = WC.CASES[name]
    h, m, mask = _tensors(case)
    for connectivity in WC.CONNECTIVITIES[case.dims]:
        where, label = case.unambiguous(connectivity)
        got, seed = watershed(h, m, mask=mask, connectivity=connectivity, dims=case.dims, return_seed=True)
        assert np.array_equal(got.numpy()[where], label[where]), (name, connectivity)
        assert np.array_equal(case.expected(connectivity)[0][where], label[where]), (name, connectivity)
        reached = seed.numpy() >= 0
        share = where[reached].mean()
        print(f"{name} connectivity {connectivity}: {100 * share:.1f} % of {int(reached.sum())} reached positions are unambiguous")
        if name == "blobs_edt":
            assert share >= 0.9, share


@pytest.mark.parametrize("connectivity", (4, 8))
def test_constant_landscape_is_breadth_first_search(connectivity):
    case = WC.CASES["constant"]
    h, m, mask = _tensors(case)
    labels, seed = WC.bfs_expected(case.markers, case.flooded, connectivity == 8)
    got = watershed(h, m, mask=mask, connectivity=connectivity, return_seed=True)
    assert np.array_equal(got[0].numpy(), labels) and np.array_equal(got[1].numpy(), seed)
    assert np.array_equal(case.expected(connectivity)[0], labels) and np.array_equal(case.expected(connectivity)[2], seed)


@pytest.mark.parametrize("connectivity", (4, 8))
def test_two_disc_split(connectivity):
    """the recipe of the module docstring on two overlapping discs: one component becomes two instances"""
    sem, truth = NC.two_discs()
    t = torch.from_numpy(sem)
    cores, n = connected_components(distance_transform(t) > 8)
    assert int(n) == 2
    inst = watershed(-distance_transform(t), cores, mask=t != 0, connectivity=connectivity)
    assert inst.dtype == torch.int32 and int((inst != 0).sum()) == 573 == int(sem.sum()) and sorted(np.unique(inst.numpy())) == [0, 1, 2]
    assert torch.equal(inst != 0, t != 0)
    res = match_instances(inst, torch.from_numpy(truth), thresholds=(0.5,), num_pred=2, num_truth=2)
    assert int(res["tp"][0]) == 2 and int(res["fp"][0]) == 0 and int(res["fn"][0]) == 0
    assert bool((res["pred_iou"] >= 0.9).all()), res["pred_iou"]


def test_height_dtypes_and_out():
    case = WC.CASES["u8_noise_holes"]
    h, m, mask = _tensors(case)
    want = watershed(h, m, mask=mask)
    for dtype in (torch.float32, torch.float16, torch.bfloat16, torch.int16):
        assert torch.equal(watershed(h.to(dtype), m, mask=mask), want), dtype
    assert torch.equal(watershed(h, m, mask=mask.to(torch.uint8) * 5), want)
    for dtype in (torch.int16, torch.int32, torch.int64):
        assert torch.equal(watershed(h, m.to(dtype), mask=mask), want.to(dtype))
    assert torch.equal(watershed(h, m != 0, mask=mask), want != 0)
    out = torch.empty_like(m)
    assert watershed(h, m, mask=mask, out=out) is out and torch.equal(out, want)
    own = m.clone()
    assert watershed(h, own, mask=mask, out=own) is own and torch.equal(own, want)
    turned = watershed(h.t(), m.t(), mask=mask.t())                            # (the linear index, and with it the ties, turn with the map)
    assert torch.equal(turned, watershed(h.t().contiguous(), m.t().contiguous(), mask=mask.t().contiguous())) and not torch.equal(turned, want.t())


def test_argument_errors():
    h = torch.zeros((4, 5))
    m = torch.zeros((4, 5), dtype=torch.int32)
    with pytest.raises(TypeError, match="height must be a tensor"):
        watershed(np.zeros((4, 5), np.float32), m)
    for bad in (torch.float64, torch.int32, torch.int64, torch.bool):
        with pytest.raises(TypeError, match=r"\.float\(\)"):
            watershed(h.to(bad), m)
    with pytest.raises(TypeError, match="markers must be a tensor"):
        watershed(h, np.zeros((4, 5), np.int32))
    with pytest.raises(TypeError, match="integer labels"):
        watershed(h, m.float())
    with pytest.raises(ValueError, match="dims must be 2 or 3"):
        watershed(h, m, dims=4)
    with pytest.raises(ValueError, match=r"\[\*stack, D, H, W\]"):
        watershed(h, m, dims=3, connectivity=6)
    for dims, bad in ((2, 6), (2, True), (3, 8), (2, 26)):
        with pytest.raises(ValueError, match="connectivity must be"):
            watershed(h[None], m[None], dims=dims, connectivity=bad)
    with pytest.raises(TypeError, match="background"):
        watershed(h, m, background=None)
    with pytest.raises(TypeError, match="background"):
        watershed(h, m, background=0.5)
    with pytest.raises(ValueError, match="height must have shape"):
        watershed(torch.zeros((5, 4)), m)
    with pytest.raises(ValueError, match="height must have shape"):
        watershed(torch.zeros((4, 5), device="meta"), m)
    with pytest.raises(TypeError, match="mask must be bool or uint8"):
        watershed(h, m, mask=torch.ones((4, 5), dtype=torch.int32))
    with pytest.raises(TypeError, match="mask must be a tensor"):
        watershed(h, m, mask=np.ones((4, 5), bool))
    with pytest.raises(ValueError, match="mask must have shape"):
        watershed(h, m, mask=torch.ones((5, 4), dtype=torch.bool))
    for bad in (0, -3, 1 << 31):
        with pytest.raises(ValueError, match="max_sweeps"):
            watershed(h, m, max_sweeps=bad)
    with pytest.raises(TypeError, match="max_sweeps"):
        watershed(h, m, max_sweeps=2.0)
    for out in (torch.zeros((4, 5), dtype=torch.int64), torch.zeros((5, 4), dtype=torch.int32), torch.zeros((4, 5), dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError, match="out must be"):
            watershed(h, m, out=out)
    with pytest.raises(TypeError, match="out must be"):
        watershed(h, m, out=np.zeros((4, 5), np.int32))
    one = torch.zeros(1, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"2\^31 - 2"):
        watershed(one.expand(1 << 16, 1 << 15), one.expand(1 << 16, 1 << 15))


def test_empty_inputs():
    before = N.calls
    got = watershed(torch.zeros((3, 0, 5)), torch.zeros((3, 0, 5), dtype=torch.int16), return_cost=True, return_seed=True, return_sweeps=True)
    assert got[0].shape == (3, 0, 5) and got[0].dtype == torch.int16 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32 and got[3] == (0, 0)
    out = torch.zeros((0, 2, 2), dtype=torch.int64)
    assert watershed(torch.zeros((0, 2, 2), dtype=torch.uint8), out.clone(), dims=3, connectivity=26, out=out) is out
    assert N.calls == before


# ---------------------------------------------------------------------------------------------------------------- native, host only
COST, SEED = 1, 2


def _plan(lib, dims, B, D, H, W, flags=0):
    nbytes = ctypes.c_int64(-1)
    return lib.ptb_watershed_plan(dims, B, D, H, W, flags, ctypes.byref(nbytes)), nbytes.value


def _up16(v):
    return (v + 15) // 16 * 16


def test_plan_workspace_over_a_sweep_of_extents():
    """16 bytes per position (height key, cost key, path key), 12 per tile (seed flag, two sweep flags), 16 of sweep words"""
    lib = N.load()
    for dims, B, D, H, W in [(2, 1, 1, 1, 1), (2, 3, 1, 17, 65), (2, 1, 1, 5000, 5000), (2, 64, 1, 512, 512), (2, 5_000_000, 1, 1, 1), (2, 1, 1, 64, 64), (2, 1, 1, 65, 129),
                             (3, 1, 1, 1, 1), (3, 2, 5, 9, 33), (3, 1, 256, 256, 256), (3, 4, 9, 17, 23)]:
        n = B * D * H * W
        tiles = B * -(-H // 64) * -(-W // 64) if dims == 2 else B * -(-D // 8) * -(-H // 8) * -(-W // 32)
        for flags in (0, COST, SEED, COST | SEED):
            rc, nbytes = _plan(lib, dims, B, D, H, W, flags)
            assert rc == 0 and nbytes == 16 + 3 * _up16(4 * tiles) + 2 * _up16(4 * n) + _up16(8 * n), (dims, B, D, H, W, flags)
    assert lib.ptb_watershed_plan(2, 1, 1, 4, 4, 0, None) == 0


def test_entry_points_refuse_bad_arguments_without_a_device():
    """The entry points validate before they touch the device, so these calls are safe without a GPU."""
    lib = N.load()
    assert _plan(lib, 4, 1, 1, 4, 4)[0] == -1 and _plan(lib, 2, 1, 2, 4, 4)[0] == -1 and _plan(lib, 2, 0, 1, 4, 4)[0] == -1 and _plan(lib, 3, 1, 4, 0, 4)[0] == -1
    assert _plan(lib, 2, 1, 1, 1 << 16, 1 << 15)[0] == N.PTB_EUNSUPPORTED and _plan(lib, 3, 2, 1 << 10, 1 << 10, 1 << 10)[0] == N.PTB_EUNSUPPORTED
    assert _plan(lib, 2, 1, 1, 3, 46341)[0] == 0                                 # (no squared distances here: only the number of positions is limited)
    assert _plan(lib, 2, 1, 1, 4, 4, 4)[0] == -1 and _plan(lib, 2, 1, 1, 4, 4, -1)[0] == -1      # unknown flags
    fake = ctypes.c_void_p(4096)                      # (never dereferenced: every call below is refused first)
    odd = ctypes.c_void_p(4100)
    big = 1 << 40
    took = (ctypes.c_int * 2)(5, 5)

    def ws(height=fake, hd=N.F32, markers=fake, mb=4, mask=None, dims=2, B=1, D=1, H=4, W=4, conn=8, bg=0, fill=0, flags=0, max_sweeps=100, labels=ctypes.c_void_p(8192),
           cost=None, seed=None, sweeps=took, work=fake, nbytes=big):
        return lib.ptb_watershed(height, hd, markers, mb, mask, dims, B, D, H, W, conn, bg, fill, flags, max_sweeps, labels, cost, seed, sweeps, work, nbytes, None)

    assert ws(height=None) == -1 and ws(markers=None) == -1 and ws(labels=None) == -1 and ws(work=None) == -1
    assert list(took) == [-1, -1]
    assert ws(hd=N.U16) == -1 and ws(hd=-1) == -1 and ws(hd=6) == -1            # height element types
    assert ws(mb=3) == -1 and ws(mb=0) == -1 and ws(mb=16) == -1                # marker element size
    assert ws(dims=1) == -1 and ws(dims=2, D=2) == -1 and ws(H=0) == -1         # dims, extents
    assert ws(conn=6) == -1 and ws(conn=0) == -1 and ws(dims=3, D=2, conn=8) == -1 and ws(dims=3, D=2, conn=4) == -1
    assert ws(flags=4) == -1 and ws(flags=COST) == -1 and ws(cost=fake) == -1 and ws(flags=SEED) == -1 and ws(seed=fake) == -1     # flags and pointers disagree
    assert ws(max_sweeps=0) == -1 and ws(max_sweeps=-1) == -1
    assert ws(H=1 << 16, W=1 << 15) == N.PTB_EUNSUPPORTED
    need = _plan(lib, 2, 1, 1, 4, 4)[1]
    assert ws(nbytes=need - 1) == -1 and ws(work=odd) == -1 and ws(labels=odd) == -1
    assert ws(flags=COST, cost=odd) == -1 and ws(flags=SEED, seed=odd) == -1
    assert ws(labels=fake) == -1                                                 # the labels may not be written over the markers
    assert N._ERR[N.PTB_ENOTCONVERGED].startswith("the relaxation did not converge") and N.PTB_ENOTCONVERGED == -7
