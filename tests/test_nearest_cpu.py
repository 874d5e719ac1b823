"""CPU: the host form of utils.nearest equals the brute-force restatements of tests/nearest_cases.py -- the index exactly, smallest linear
index on a tie -- and names a site at scipy's distance on every case; ``return_distance`` has the bits of ``distance_transform``; the label
expansion equals its definition; arguments are validated; the native entry points plan consistently and refuse bad arguments without
a device."""
import ctypes

import numpy as np
import pytest
import torch

import distance_cases as DC
import nearest_cases as NC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import connected_components, distance_transform, expand_labels, match_instances, nearest_site


@pytest.mark.parametrize("name", NC.SMALL)
def test_host_form_equals_the_brute_force(name):
    a, dims = NC.CASES[name]
    want = NC.expected_index(name)
    before = N.calls
    got = nearest_site(torch.from_numpy(a), dims=dims)
    assert got.dtype == torch.int32 and got.shape == a.shape and np.array_equal(got.numpy(), want), name
    for e, s in zip(DC._entries(got.numpy(), dims), DC._entries(a == 0, dims)):
        assert bool((e >= 0).all()) if s.any() else bool((e == -1).all()), name
    entries = len(DC._entries(a, dims))
    rows, cols = np.nonzero((a == 0).reshape(entries, -1))
    assert np.array_equal(got.numpy().reshape(entries, -1)[rows, cols], cols), "a site gets its own index"
    assert torch.equal(nearest_site(torch.from_numpy(a != 0), dims=dims), got) and torch.equal(nearest_site(torch.from_numpy(a.astype(np.int64)), dims=dims), got)
    assert N.calls == before, "a CPU tensor reached the native library"


@pytest.mark.parametrize("name", list(NC.CASES))
def test_host_form_names_a_nearest_site(name):
    """validity against scipy's distances, the four cases above the brute-force limit included"""
    a, dims = NC.CASES[name]
    if not (a == 0).any():
        assert bool((nearest_site(torch.from_numpy(a), dims=dims) == -1).all())
        return
    from scipy.ndimage import distance_transform_edt  # noqa: F401  (the yardstick of check_valid's large cases)

    NC.check_valid(nearest_site(torch.from_numpy(a), dims=dims).numpy(), name)


@pytest.mark.parametrize("name", DC.FOREGROUND_CASES)
def test_foreground_rule(name):
    a, dims = NC.CASES[name]
    t = torch.from_numpy(a)
    for c in list(range(int(a.max()) + 2)) + [300, -1]:
        got = nearest_site(t, foreground=c, dims=dims)
        assert np.array_equal(got.numpy(), NC.brute_nearest(a != c, dims)[1]), (name, c)
        assert torch.equal(nearest_site(t, foreground=c, background=None, dims=dims), got)
    assert bool((nearest_site(t, background=300) == -1).all()), "a background that occurs nowhere: no site"
    assert np.array_equal(nearest_site(t, background=1).numpy(), NC.brute_nearest(a == 1, dims)[1])


@pytest.mark.parametrize("spacing", NC.EXACT_SPACINGS, ids=str)
@pytest.mark.parametrize("name", NC.EXACT_SPACING_CASES)
def test_host_form_with_exact_spacing(name, spacing):
    a, dims = NC.CASES[name]
    got = nearest_site(torch.from_numpy(a), dims=dims, spacing=spacing[-dims:])
    assert np.array_equal(got.numpy(), NC.expected_index_spacing(name, spacing)), (name, spacing)


@pytest.mark.parametrize("name", ("blobs", "stack_hole", "volume_stack_hole", "len257_z3", "wide_one_site"))
def test_return_distance_has_the_bits_of_distance_transform(name):
    a, dims = NC.CASES[name]
    t = torch.from_numpy(a)
    for kw in (dict(), dict(spacing=DC.SPACINGS[0][-dims:]), dict(spacing=NC.EXACT_SPACINGS[0][-dims:]), dict(foreground=1)):
        index, sq = nearest_site(t, dims=dims, return_distance=True, **kw)
        want = distance_transform(t, dims=dims, squared=True, **kw)
        assert sq.dtype == want.dtype and np.array_equal(sq.numpy().view(np.int32), want.numpy().view(np.int32)), (name, kw)
        assert torch.equal(index, nearest_site(t, dims=dims, **kw))
    out = torch.full(a.shape, 7, dtype=torch.int32)
    index, sq = nearest_site(t, dims=dims, return_distance=True, out=out)
    assert index is out and torch.equal(out, nearest_site(t, dims=dims))


@pytest.mark.parametrize("case", NC.EXPANSIONS, ids=repr)
def test_expansion_host_form_equals_the_definition(case):
    m = torch.from_numpy(case.markers)
    mask = None if case.mask is None else torch.from_numpy(case.mask)
    before = N.calls
    got = expand_labels(m, distance=case.distance, mask=mask, background=case.background, dims=case.dims, spacing=case.spacing)
    assert got.dtype == m.dtype and got.shape == m.shape and np.array_equal(got.numpy(), case.expected), case
    if mask is not None:
        assert torch.equal(expand_labels(m, distance=case.distance, mask=mask.to(torch.uint8) * 5, background=case.background, dims=case.dims, spacing=case.spacing), got)
    out = torch.empty_like(m)
    assert expand_labels(m, distance=case.distance, mask=mask, background=case.background, dims=case.dims, spacing=case.spacing, out=out) is out
    assert torch.equal(out, got) and N.calls == before


def test_expansion_by_zero_is_the_identity_and_the_cases_expand():
    grown = 0
    for case in NC.EXPANSIONS:
        m = torch.from_numpy(case.markers)
        assert torch.equal(expand_labels(m, distance=0, background=case.background, dims=case.dims, spacing=case.spacing), m), case
        grown += int((case.expected != case.markers).sum())
    assert grown > 10_000, "the expansion cases hardly expand anything"


def test_two_disc_split():
    """the recipe of the module docstring on two overlapping discs: one component becomes two instances"""
    sem, truth = NC.two_discs()
    t = torch.from_numpy(sem)
    assert int(connected_components(t)[1]) == 1
    cores, n = connected_components(distance_transform(t) > 8)
    assert int(n) == 2
    inst = expand_labels(cores, mask=t != 0)
    assert inst.dtype == torch.int32 and int((inst != 0).sum()) == 573 == int(sem.sum()) and sorted(np.unique(inst.numpy())) == [0, 1, 2]
    assert torch.equal(inst != 0, t != 0)
    res = match_instances(inst, torch.from_numpy(truth), thresholds=(0.5,), num_pred=2, num_truth=2)
    assert int(res["tp"][0]) == 2 and int(res["fp"][0]) == 0 and int(res["fn"][0]) == 0
    assert bool((res["pred_iou"] >= 0.9).all()), res["pred_iou"]
    from scipy.ndimage import distance_transform_edt, label

    host_cores, _ = label(distance_transform_edt(sem) > 8, structure=np.ones((3, 3)))
    idx = distance_transform_edt(host_cores == 0, return_distances=False, return_indices=True)
    host = np.where(sem != 0, host_cores[tuple(idx)], 0)
    assert sorted(np.bincount(host.ravel())[1:]) == [279, 294]


def test_argument_errors():
    t = torch.zeros((4, 5), dtype=torch.uint8)
    with pytest.raises(TypeError, match="integer labels"):
        nearest_site(t.float())
    with pytest.raises(TypeError):
        nearest_site(np.zeros((4, 5), np.uint8))
    with pytest.raises(ValueError, match="dims must be 2 or 3"):
        nearest_site(t, dims=1)
    with pytest.raises(ValueError, match=r"\[\*stack, D, H, W\]"):
        nearest_site(t, dims=3)
    with pytest.raises(ValueError, match="needs foreground"):
        nearest_site(t, background=None)
    with pytest.raises(TypeError, match="background"):
        nearest_site(t, background=0.5)
    with pytest.raises(ValueError, match="spacing"):
        nearest_site(t, spacing=(1.0, 0.0))
    for out in (torch.zeros((4, 5), dtype=torch.int64), torch.zeros((5, 4), dtype=torch.int32), torch.zeros((4, 5), dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError, match="out must be"):
            nearest_site(t, out=out)
    with pytest.raises(TypeError, match="out must be"):
        nearest_site(t, out=np.zeros((4, 5), np.int32))
    one = torch.zeros(1, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"2\^31 - 2"):
        nearest_site(one.expand(1 << 16, 1 << 15))
    with pytest.raises(ValueError, match=r"H\^2 \+ W\^2"):
        nearest_site(one.expand(3, 46341))
    with pytest.raises(ValueError, match=r"D\^2 \+ H\^2 \+ W\^2"):
        nearest_site(one.expand(33000, 33000, 1), dims=3)

    m = torch.zeros((4, 5), dtype=torch.int32)
    with pytest.raises(TypeError, match="integer labels"):
        expand_labels(m.float())
    with pytest.raises(TypeError, match="markers must be a tensor"):
        expand_labels(np.zeros((4, 5), np.int32))
    with pytest.raises(ValueError, match="dims must be 2 or 3"):
        expand_labels(m, dims=4)
    with pytest.raises(ValueError, match=r"\[\*stack, D, H, W\]"):
        expand_labels(m, dims=3)
    with pytest.raises(TypeError, match="background"):
        expand_labels(m, background=None)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="distance must be finite"):
            expand_labels(m, distance=bad)
    for bad in ("3", True, (1.0,)):
        with pytest.raises(TypeError, match="distance must be"):
            expand_labels(m, distance=bad)
    with pytest.raises(TypeError, match="mask must be bool or uint8"):
        expand_labels(m, mask=torch.ones((4, 5), dtype=torch.int32))
    with pytest.raises(TypeError, match="mask must be a tensor"):
        expand_labels(m, mask=np.ones((4, 5), bool))
    with pytest.raises(ValueError, match="mask must have shape"):
        expand_labels(m, mask=torch.ones((5, 4), dtype=torch.bool))
    with pytest.raises(ValueError, match="mask must have shape"):
        expand_labels(m, mask=torch.ones((4, 5), dtype=torch.bool, device="meta"))
    for out in (torch.zeros((4, 5), dtype=torch.int64), torch.zeros((5, 4), dtype=torch.int32), torch.zeros((4, 5), dtype=torch.int32, device="meta")):
        with pytest.raises(ValueError, match="out must be"):
            expand_labels(m, out=out)
    with pytest.raises(ValueError, match="spacing"):
        expand_labels(m, spacing=(1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match=r"2\^31 - 2"):
        expand_labels(one.expand(1 << 16, 1 << 15))
    with pytest.raises(ValueError, match=r"H\^2 \+ W\^2"):
        expand_labels(one.expand(3, 46341))


def test_empty_inputs():
    before = N.calls
    d = nearest_site(torch.zeros((3, 0, 5), dtype=torch.int16))
    assert d.shape == (3, 0, 5) and d.dtype == torch.int32
    index, sq = nearest_site(torch.zeros((0, 5), dtype=torch.uint8), return_distance=True, spacing=(1.0, 2.0))
    assert index.dtype == torch.int32 and sq.dtype == torch.float32 and sq.shape == (0, 5)
    assert nearest_site(torch.zeros((0, 5), dtype=torch.uint8), return_distance=True)[1].dtype == torch.int32
    out = torch.zeros((0, 2, 2), dtype=torch.int32)
    assert nearest_site(torch.zeros((0, 2, 2), dtype=torch.bool), dims=3, out=out) is out
    e = expand_labels(torch.zeros((2, 0, 3), dtype=torch.int64), distance=2.0, mask=torch.zeros((2, 0, 3), dtype=torch.bool))
    assert e.shape == (2, 0, 3) and e.dtype == torch.int64
    assert N.calls == before


# ---------------------------------------------------------------------------------------------------------------- native, host only
INDEX, SQUARED, GATHER, MAX_SQ = 1, 2, 4, 8


def _plan(lib, dims, B, D, H, W, flags=INDEX):
    nbytes = ctypes.c_int64(-1)
    return lib.ptb_nearest_plan(dims, B, D, H, W, flags, ctypes.byref(nbytes)), nbytes.value


def _up16(v):
    return (v + 15) // 16 * 16


def test_plan_workspace_over_a_sweep_of_extents():
    """per position: two 32-bit stack words, and 4 bytes for every distance and feature map that is not the caller's tensor"""
    lib = N.load()
    maps = {2: {INDEX: 4, INDEX | SQUARED: 4, SQUARED: 5, GATHER: 5, GATHER | MAX_SQ: 6, GATHER | INDEX: 4, GATHER | MAX_SQ | INDEX | SQUARED: 4},
            3: {INDEX: 5, INDEX | SQUARED: 4, SQUARED: 5, GATHER: 6, GATHER | MAX_SQ: 6, GATHER | INDEX: 5, GATHER | MAX_SQ | INDEX | SQUARED: 4}}
    for dims, B, D, H, W in [(2, 1, 1, 1, 1), (2, 3, 1, 17, 65), (2, 1, 1, 5000, 5000), (2, 64, 1, 512, 512), (2, 5_000_000, 1, 1, 1), (2, 1, 1, 32767, 32767),
                             (3, 1, 1, 1, 1), (3, 2, 5, 9, 33), (3, 1, 512, 512, 512), (3, 4, 9, 17, 23)]:
        n = B * D * H * W
        for flags, count in maps[dims].items():
            rc, nbytes = _plan(lib, dims, B, D, H, W, flags)
            assert rc == 0 and nbytes == count * _up16(4 * n), (dims, B, D, H, W, flags)
    assert lib.ptb_nearest_plan(2, 1, 1, 4, 4, INDEX, None) == 0


def test_entry_points_refuse_bad_arguments_without_a_device():
    """The entry points validate before they touch the device, so these calls are safe without a GPU."""
    lib = N.load()
    assert _plan(lib, 4, 1, 1, 4, 4)[0] == -1 and _plan(lib, 2, 1, 2, 4, 4)[0] == -1 and _plan(lib, 2, 0, 1, 4, 4)[0] == -1 and _plan(lib, 3, 1, 4, 0, 4)[0] == -1
    assert _plan(lib, 2, 1, 1, 1 << 16, 1 << 15)[0] == N.PTB_EUNSUPPORTED and _plan(lib, 3, 2, 1 << 10, 1 << 10, 1 << 10)[0] == N.PTB_EUNSUPPORTED
    assert _plan(lib, 2, 1, 1, 3, 46341)[0] == N.PTB_EUNSUPPORTED and _plan(lib, 2, 1, 1, 3, 46340)[0] == 0
    assert _plan(lib, 3, 1, 33000, 33000, 1)[0] == N.PTB_EUNSUPPORTED and _plan(lib, 2, 33000, 1, 33000, 1)[0] == 0
    assert _plan(lib, 2, 1, 1, 4, 4, 0)[0] == -1 and _plan(lib, 2, 1, 1, 4, 4, 16)[0] == -1 and _plan(lib, 2, 1, 1, 4, 4, MAX_SQ)[0] == -1      # asks for nothing
    assert _plan(lib, 2, 1, 1, 4, 4, MAX_SQ | INDEX)[0] == -1                                                                       # a limit without a gather
    fake = ctypes.c_void_p(4096)                      # (never dereferenced: every call below is refused first)
    odd = ctypes.c_void_p(4100)
    big = 1 << 40
    sp = (ctypes.c_double * 3)(1.0, 1.0, 1.0)

    def near(labels=fake, eb=1, dims=2, B=1, D=1, H=4, W=4, rule=0, value=0, spacing=None, flags=INDEX, index=fake, squared=None, gather=None, mask=None,
             max_sq=0.0, ws=fake, nbytes=big):
        return lib.ptb_nearest(labels, eb, dims, B, D, H, W, rule, value, spacing, flags, index, squared, gather, mask, max_sq, ws, nbytes, None)

    assert near(labels=None) == -1 and near(ws=None) == -1
    assert near(eb=3) == -1 and near(eb=0) == -1                                # element size
    assert near(dims=1) == -1 and near(dims=2, D=2) == -1 and near(H=0) == -1   # dims, extents
    assert near(rule=2) == -1 and near(rule=-1) == -1                           # site rule
    assert near(flags=0, index=None) == -1 and near(flags=16) == -1             # nothing asked for; an unknown flag
    assert near(index=None) == -1 and near(squared=fake) == -1 and near(gather=fake) == -1 and near(flags=INDEX | SQUARED) == -1      # pointers and flags disagree
    assert near(mask=fake) == -1                                                # a mask without a gather
    assert near(flags=GATHER, index=None, gather=fake, rule=0) == -1            # the labelled positions are the sites
    assert near(flags=GATHER | MAX_SQ, index=None, gather=fake, rule=1, max_sq=-1.0) == -1 and near(flags=GATHER | MAX_SQ, index=None, gather=fake, rule=1, max_sq=float("nan")) == -1
    for bad in ((1.0, 0.0, 1.0), (1.0, 1.0, -1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, float("inf"))):
        assert near(spacing=(ctypes.c_double * 3)(*bad)) == -1
    assert near(dims=3, D=4, spacing=(ctypes.c_double * 3)(0.0, 1.0, 1.0)) == -1 and near(dims=2, nbytes=0, spacing=sp) == -1
    assert near(H=1 << 16, W=1 << 15) == N.PTB_EUNSUPPORTED and near(H=3, W=46341) == N.PTB_EUNSUPPORTED
    need = _plan(lib, 2, 1, 1, 4, 4)[1]
    assert near(nbytes=need - 1) == -1 and near(ws=odd) == -1 and near(index=odd) == -1        # workspace too small, misaligned; out misaligned
    assert near(flags=INDEX | SQUARED, squared=odd) == -1 and near(flags=GATHER, index=None, gather=odd, rule=1) == -1
    need_g, need_gm = _plan(lib, 2, 1, 1, 4, 4, GATHER)[1], _plan(lib, 2, 1, 1, 4, 4, GATHER | MAX_SQ)[1]
    assert need_gm > need_g and near(flags=GATHER | MAX_SQ, index=None, gather=fake, rule=1, nbytes=need_g) == -1
