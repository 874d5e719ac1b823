"""CPU: the deferred slab merge of VolumeMerger(crops=, defer=True) without a device -- the host-side plan (ptb_volume_plan_create
through its host-readable item table) against brute force in numpy, the argument validation of the new entry points, and the torch-op
merger serving the same interface."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__ as g
from volume_defer_cases import cases, cover_lists, wide_slab

CASES = cases()
KINDS = [(torch.float32, False), (torch.uint8, False), (torch.uint8, True), (torch.int64, True), (torch.float16, False), (torch.bfloat16, False)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    g.build()


def _plan(case, channels=3):
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumePlan

    return VolumePlan(case["crops"], case["tile"], case["shape"], channels, case["window"])


def _check_plan(case):
    plan = _plan(case)
    items, info, last = plan.items(), plan.group_info, plan.last_group_of_tile
    cover, _count = cover_lists(case)
    z0, y0, x0, od, oh, ow = case["window"]
    n = len(case["crops"])
    seen = np.zeros(case["shape"], dtype=np.int64)
    group_tiles = [set() for _ in range(plan.n_groups)]
    group_items = np.zeros(plan.n_groups, dtype=np.int64)
    for row in items:
        grp, a0, a1, b0, b1, c0, c1, nt = (int(v) for v in row[:8])
        assert a0 < a1 and b0 < b1 and c0 < c1
        box = (slice(a0, a1), slice(b0, b1), slice(c0, c1))
        seen[box] += 1
        # the covering list of every voxel of the box, in integration order, is the item's
        assert (cover[box] == row[8:16]).all(), row
        assert nt == int((row[8:16] >= 0).sum())
        assert info[grp, 0] <= a0 and a1 <= info[grp, 1]            # an item lies in its group's slab
        group_tiles[grp].update(int(t) for t in row[8:8 + nt])
        group_items[grp] += 1
    # items tile the window exactly once, and nothing outside it
    want = np.zeros(case["shape"], dtype=np.int64)
    want[z0:z0 + od, y0:y0 + oh, x0:x0 + ow] = 1
    assert (seen == want).all()
    # groups: items contiguous in launch order, heavy first; completing tile; launch order = ascending completing tile
    assert (np.diff(items[:, 0]) >= 0).all()
    for grp in range(plan.n_groups):
        mine = items[items[:, 0] == grp]
        assert (np.diff(mine[:, 7]) <= 0).all()
        assert info[grp, 3] == group_items[grp] == len(mine) > 0
        assert info[grp, 2] == (max(group_tiles[grp]) if group_tiles[grp] else 0)
        assert len(group_tiles[grp]) <= 224
    assert (np.diff(info[:, 2]) >= 0).all()
    # a slab is complete when its last covering tile is in: the groups of one slab end with exactly that tile
    for s0, s1 in sorted({(int(r[0]), int(r[1])) for r in info}):
        inside = cover[max(s0, z0):min(s1, z0 + od), y0:y0 + oh, x0:x0 + ow]
        assert max(0, int(inside.max())) == max(int(r[2]) for r in info if (int(r[0]), int(r[1])) == (s0, s1))
    assert plan.n_slabs == len({(int(r[0]), int(r[1])) for r in info})
    # last_group_of_tile and the custody peak, by direct simulation
    sim_last = [max([grp for grp in range(plan.n_groups) if t in group_tiles[grp]], default=-1) for t in range(n)]
    assert sim_last == [int(v) for v in last]
    until = [max(t, int(info[sim_last[t], 2])) if sim_last[t] >= 0 else t for t in range(n)]
    peak = max(sum(1 for s in range(t + 1) if until[s] >= t) for t in range(n))
    assert plan.peak_held_tiles == peak
    return plan


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_against_brute_force(name):
    plan = _check_plan(CASES[name])
    assert plan.vec_ok == (name != "off_grid")


def test_plan_cuts_a_wide_slab_into_launch_groups():
    plan = _check_plan(wide_slab())
    assert plan.n_groups > plan.n_slabs


def test_half_overlap_holds_two_layers():
    """z-major crops: the tiles of two z-layers are in custody when a slab between them completes."""
    case = CASES["half_overlap"]
    assert _plan(case).peak_held_tiles == 2 * 2 * 2


def test_window_smaller_than_the_volume_drops_items():
    case = dict(CASES["half_overlap"], window=(3, 5, 6, 20, 9, 11))
    plan = _check_plan(case)
    assert (plan.last_group_of_tile == -1).any()         # tiles nobody reads are not held for anything


def test_quarter_step_is_refused():
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumePlan, VolumeSlicer

    s = VolumeSlicer((32, 32, 32), 16, 4)
    with pytest.raises(NotImplementedError, match="8 tiles"):
        VolumePlan(s.crops, (16, 16, 16), s.target_shape, 2)


def test_argument_validation_without_gpu():
    from pytorch_toolbelt_amd import _native as N

    lib = N.load()
    one = N.i64_array([0])
    win = N.i64_array([0, 0, 0, 8, 8, 8])
    out = ctypes.c_void_p()
    ok = lambda *a: lib.ptb_volume_plan_create(*a, ctypes.byref(out))   # noqa: E731
    assert lib.ptb_volume_plan_create(None, one, one, 1, 1, 8, 8, 8, 8, 8, 8, win, 0, 0, ctypes.byref(out)) == -1
    assert lib.ptb_volume_plan_create(one, one, one, 1, 1, 8, 8, 8, 8, 8, 8, None, 0, 0, ctypes.byref(out)) == -1
    assert lib.ptb_volume_plan_create(one, one, one, 1, 1, 8, 8, 8, 8, 8, 8, win, 0, 0, None) == -1
    assert ok(one, one, one, 0, 1, 8, 8, 8, 8, 8, 8, win, 0, 0) == -1        # no tiles
    assert ok(one, one, one, 1, 0, 8, 8, 8, 8, 8, 8, win, 0, 0) == -1        # no channels
    assert ok(one, one, one, 1, 1, 8, 0, 8, 8, 8, 8, win, 0, 0) == -1        # empty tile
    assert ok(one, one, one, 1, 1, 8, 8, 8, 8, 8, 8, win, 2, 0) == -1        # layout
    assert ok(one, one, one, 1, 1, 8, 8, 8, 8, 8, 8, win, 0, 6) == -1        # kind
    assert ok(one, one, one, 1, 1, 8, 8, 8, 8, 8, 7, win, 0, 0) == -4        # tile / window outside the volume
    assert ok(N.i64_array([1]), one, one, 1, 1, 8, 8, 8, 8, 8, 8, win, 0, 0) == -4
    assert ok(one, one, one, 1, 1, 8, 8, 8, 8, 8, 8, N.i64_array([0, 0, 0, 8, 9, 8]), 0, 0) == -4
    assert ok(one, one, one, 1, 1, 8, 8, 8, 8, 8, 8, N.i64_array([0, -1, 0, 8, 8, 8]), 0, 0) == -1
    assert ok(one, one, one, 1, 300, 8, 8, 8, 8, 8, 8, win, 0, N.CROP_ARGMAX_U8) == -2
    assert ok(one, one, one, 1, 2, 8, 8, 8, 8, 8, 8, win, 0, 0) == 96 * 1 and out.value
    plan = out
    masks = N.int_array([0, 1])
    fake = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused before anything touches the device
    sub = lambda *a: lib.ptb_volume_plan_submit(*a, None)   # noqa: E731
    assert sub(None, 0, 1, fake, 512, 512, 0, 0, None, 0, fake, fake) == -1
    assert sub(plan, 0, 1, None, 512, 512, 0, 0, None, 0, fake, fake) == -1
    assert sub(plan, 0, 1, fake, 512, 512, 0, 0, None, 0, None, fake) == -1
    assert sub(plan, 0, 1, fake, 512, 512, 0, 0, None, 0, fake, None) == -1
    assert sub(plan, 0, 0, fake, 512, 512, 0, 0, None, 0, fake, fake) == -1       # empty batch
    assert sub(plan, 0, 1, fake, 0, 512, 0, 0, None, 0, fake, fake) == -1         # tile stride
    assert sub(plan, 0, 1, fake, 512, 512, 3, 0, None, 0, fake, fake) == -1       # dtype
    assert sub(plan, 0, 1, fake, 512, 512, 0, 9, masks, 1, fake, fake) == -1      # views
    assert sub(plan, 0, 1, fake, 512, 512, 0, 2, None, 1, fake, fake) == -1       # views without masks
    assert sub(plan, 0, 1, fake, 512, 512, 0, 2, N.int_array([0, 8]), 1, fake, fake) == -1
    assert sub(plan, 0, 1, fake, 512, 512, 0, 2, masks, 7, fake, fake) == -1      # reduction
    assert sub(plan, 0, 1, fake, 512, 512, 0, 0, None, 0, fake, fake) == -1       # no table uploaded yet
    assert lib.ptb_volume_plan_upload(plan, None, None) == -1
    assert lib.ptb_volume_plan_upload(None, fake, None) == -1
    assert lib.ptb_volume_plan_upload(plan, ctypes.c_void_p(4100), None) == -1    # alignment
    assert lib.ptb_volume_plan_items(None, None, 0) == -1 and lib.ptb_volume_plan_items(plan, None, 0) == 1
    assert lib.ptb_volume_plan_items(plan, N.i64_array([0] * 16), 0) == -1        # capacity
    assert lib.ptb_volume_plan_info(None, None, None, None, None, None, None, None) == -1
    assert lib.ptb_volume_plan_reset(None) == -1 and lib.ptb_volume_plan_state(None, None, None) == -1
    pos, done = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.ptb_volume_plan_state(plan, ctypes.byref(pos), ctypes.byref(done)) == 0 and (pos.value, done.value) == (0, 0)
    lib.ptb_volume_plan_destroy(plan)


# ------------------------------------------------------------------------------------------------ the torch-op merger
def _host_pair(case, channels, result, dtype=torch.float64):
    from pytorch_toolbelt_amd.inference.tiles_3d import HostBackedVolumeMerger, VolumeMerger

    plain = VolumeMerger(case["shape"], channels, case["weight"], device="cpu", dtype=dtype)
    deferred = VolumeMerger(case["shape"], channels, case["weight"], device="cpu", dtype=dtype, crops=case["crops"], defer=True, result=result)
    assert type(plain) is type(deferred) is HostBackedVolumeMerger
    return plain, deferred


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0))


@pytest.mark.parametrize("layout", ["cdhw", "dhwc"])
@pytest.mark.parametrize("dtype, argmax", KINDS)
@pytest.mark.parametrize("name", ["asymmetric_pad", "gap"])
def test_host_merger_serves_every_kind_and_layout(name, dtype, argmax, layout):
    case = CASES[name]
    C, crops = 3, case["crops"]
    spec = dict(crop=case["window"], layout=layout, dtype=dtype, argmax=argmax)
    plain, deferred = _host_pair(case, C, spec)
    tiles = torch.rand((len(crops), C) + case["tile"], dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 200
    for b0 in range(0, len(crops), 4):
        plain.integrate_batch(tiles[b0:b0 + 4], crops[b0:b0 + 4])
        deferred.integrate_batch(tiles[b0:b0 + 4], crops[b0:b0 + 4])
    assert _same(deferred.merge_crop(**spec), plain.merge_crop(**spec))


def test_host_merger_default_result_mirror_and_reset():
    case = CASES["half_overlap"]
    C, crops, n = 2, case["crops"], len(case["crops"])
    plain, deferred = _host_pair(case, C, None)
    assert deferred.peak_held_tiles == 0
    gen = torch.Generator().manual_seed(2)
    for image in range(2):
        views = torch.rand((2 * n, C) + case["tile"], dtype=torch.float64, generator=gen) + 0.1
        for b0 in range(0, n, 5):
            b1 = min(n, b0 + 5)
            batch = torch.cat([views[b0:b1], views[n + b0:n + b1]])
            plain.integrate_batch_deaugment(batch, crops[b0:b1], mirror="w", reduction="gmean")
            deferred.integrate_batch_deaugment(batch, crops[b0:b1], mirror="w", reduction="gmean")
        first = deferred.merge()
        assert _same(first, plain.merge())
        assert _same(deferred.merge_crop((0, 0, 0) + case["shape"]), plain.merge())      # the default spec, spelled out
        plain.reset()
        deferred.reset()
        assert float(plain.volume.abs().sum()) == 0 and float(plain.norm_mask.abs().sum()) == 0


def test_host_merger_enforces_the_contract():
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumeMerger

    case = CASES["half_overlap"]
    C, crops = 2, case["crops"]
    spec = dict(crop=case["window"], dtype=torch.uint8, argmax=True)
    _plain, deferred = _host_pair(case, C, spec)
    tiles = torch.rand((len(crops), C) + case["tile"], dtype=torch.float64)
    hint = "without defer=True"
    with pytest.raises(RuntimeError, match=hint):
        deferred.integrate_batch(tiles[1:3], crops[1:3])                       # not the next planned tiles
    deferred.integrate_batch(tiles[0:3], crops[0:3])
    with pytest.raises(RuntimeError, match=hint):
        deferred.integrate_batch(tiles[2:4], crops[2:4])                       # tile 2 again
    with pytest.raises(RuntimeError, match=hint):
        deferred.integrate_batch(tiles[3:5].float(), crops[3:5])               # dtype changed within the image
    with pytest.raises(RuntimeError, match=hint):
        deferred.integrate_batch_deaugment(torch.cat([tiles[3:5]] * 2), crops[3:5], mirror="d")
    with pytest.raises(RuntimeError, match=hint):
        deferred.merge_crop(**spec)                                            # before the last tile
    for name in ("volume", "norm_mask"):
        with pytest.raises(RuntimeError, match=hint):
            getattr(deferred, name)
    deferred.integrate_batch(tiles[3:], crops[3:])
    with pytest.raises(RuntimeError, match=hint):
        deferred.integrate_batch(tiles[:1], crops[:1])                         # past the plan
    with pytest.raises(ValueError, match="argmax=True"):
        deferred.merge()                                                       # not the default spec
    with pytest.raises(ValueError, match="argmax=True"):
        deferred.merge_crop(case["window"], dtype=torch.uint8)                 # other arguments than the spec
    assert deferred.merge_crop(**spec).dtype == torch.uint8
    # constructor: defer needs crops; crops / result need defer; unknown result keys
    with pytest.raises(ValueError, match="crops="):
        VolumeMerger(case["shape"], C, case["weight"], device="cpu", defer=True)
    with pytest.raises(ValueError, match="defer=True"):
        VolumeMerger(case["shape"], C, case["weight"], device="cpu", crops=crops)
    with pytest.raises(ValueError, match="merge_crop"):
        VolumeMerger(case["shape"], C, case["weight"], device="cpu", crops=crops, defer=True, result=dict(window=(0,) * 6))


def test_plain_host_merger_is_unchanged_and_resets():
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumeMerger

    case = CASES["step_is_size"]
    m = VolumeMerger(case["shape"], 1, case["weight"], device="cpu")
    m.integrate_batch(torch.ones((1, 1) + case["tile"]), case["crops"][:1])
    assert float(m.volume.sum()) > 0 and m.volume.shape == (1,) + case["shape"]
    m.volume = m.volume * 2                                                    # still a plain attribute
    m.reset()
    assert float(m.volume.sum()) == 0 and float(m.norm_mask.sum()) == 0
