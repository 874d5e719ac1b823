"""CPU: the host form of utils.components equals the flood fill of tests/components_cases.py on the whole case list, the flood fill
equals scipy.ndimage.label, arguments are validated, and the native entry points plan consistently and refuse bad arguments without a
device."""
import ctypes

import numpy as np
import pytest
import torch

import components_cases as C
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import component_stats, connected_components, remove_small_components

CASE_CONN = [(name, conn) for name, (_a, dims) in C.CASES.items() for conn in C.CONNECTIVITIES[dims]]


@pytest.mark.parametrize("name,conn", CASE_CONN)
def test_host_form_equals_the_flood_fill(name, conn):
    a, dims = C.CASES[name]
    want = C.expected(name, conn)
    before = N.calls
    cc, count = connected_components(torch.from_numpy(a), connectivity=conn, dims=dims)
    assert N.calls == before, "a CPU tensor reached the native library"
    assert cc.dtype == torch.int32 and cc.shape == a.shape and count.dtype == torch.int64 and count.shape == want["count"].shape
    assert np.array_equal(cc.numpy(), want["cc"]) and np.array_equal(count.numpy(), want["count"])
    if name in C.BIG_CASES:
        return
    as_bool = C.expected(name, conn, as_bool=True)
    cc_b, count_b = connected_components(torch.from_numpy(a != 0), connectivity=conn, dims=dims)
    assert np.array_equal(cc_b.numpy(), as_bool["cc"]) and np.array_equal(count_b.numpy(), as_bool["count"])
    largest = max([int(x.max()) for x in want["areas"] if x.size] or [0])
    for min_area in (1, 2, 5, largest + 1):
        got = remove_small_components(torch.from_numpy(a.astype(np.int16)), min_area, connectivity=conn, dims=dims)
        assert got.dtype == torch.int16 and np.array_equal(got.numpy(), C.remove_small(a, dims, conn, min_area, ref=want)), min_area
    if a.ndim == dims:
        n = int(want["count"])
        got = component_stats(cc, count, values=torch.from_numpy(a))
        assert np.array_equal(got["area"].numpy(), want["areas"][0]) and np.array_equal(got["bbox"].numpy(), want["boxes"][0])
        assert np.array_equal(got["value"].numpy(), want["values"][0]) and got["value"].dtype == torch.uint8
        more = component_stats(cc, max_components=n + 2)
        assert "value" not in more and np.array_equal(more["area"][:n].numpy(), want["areas"][0]) and not more["area"][n:].any() and not more["bbox"][n:].any()


@pytest.mark.parametrize("name", ["blobs", "touching", "volume_blobs"])
def test_backgrounds_of_the_host_form(name):
    a, dims = C.CASES[name]
    for conn in C.CONNECTIVITIES[dims]:
        for bg in (None, 1, 300, -1):
            want = C.restate(a, dims, conn, background=bg)
            cc, count = connected_components(torch.from_numpy(a), connectivity=conn, background=bg, dims=dims)
            assert np.array_equal(cc.numpy(), want["cc"]) and int(count) == int(want["count"]), (conn, bg)
        out = torch.from_numpy(a.copy())
        assert remove_small_components(out, 4, connectivity=conn, background=None, fill=9, dims=dims, out=out) is out
        assert np.array_equal(out.numpy(), C.remove_small(a, dims, conn, 4, background=None, fill=9))


@pytest.mark.parametrize("name,conn", [(n, c) for n, c in CASE_CONN if n not in C.BIG_CASES])
def test_flood_fill_equals_scipy(name, conn):
    ndi = pytest.importorskip("scipy.ndimage")
    a, dims = C.CASES[name]
    want = C.expected(name, conn)
    structure = ndi.generate_binary_structure(dims, dims if conn in (8, 26) else 1)
    entries = a.reshape((-1,) + a.shape[a.ndim - dims:])
    ccs = want["cc"].reshape(entries.shape)
    for e, cc in zip(entries, ccs):
        # per class, then renumbered by first position
        merged = np.zeros(e.shape, np.int64)
        offset = 0
        for v in np.unique(e[e != 0]):
            lab, n = ndi.label(e == v, structure=structure)
            merged[lab > 0] = lab[lab > 0] + offset
            offset += n
        flat = merged.reshape(-1)
        ids, first = np.unique(flat[flat > 0], return_index=True)
        renumber = np.zeros(offset + 1, np.int64)
        renumber[ids[np.argsort(first)]] = np.arange(1, ids.size + 1)
        assert np.array_equal(renumber[merged], cc), (name, conn)


def test_argument_errors():
    t = torch.zeros((4, 5), dtype=torch.uint8)
    with pytest.raises(TypeError, match="integer labels"):
        connected_components(t.float())
    with pytest.raises(TypeError):
        connected_components(np.zeros((4, 5), np.uint8))
    with pytest.raises(ValueError, match="4 or 8"):
        connected_components(t, connectivity=6)
    with pytest.raises(ValueError, match="6 or 26"):
        connected_components(t[None], connectivity=18, dims=3)
    with pytest.raises(ValueError, match="6 or 26"):
        connected_components(t[None], connectivity=8, dims=3)
    with pytest.raises(ValueError, match="dims must be 2 or 3"):
        connected_components(t, dims=1)
    with pytest.raises(ValueError, match=r"\[\*stack, D, H, W\]"):
        connected_components(t, connectivity=6, dims=3)
    with pytest.raises(TypeError, match="background"):
        connected_components(t, background=0.5)
    with pytest.raises(ValueError, match="fill is required"):
        remove_small_components(t, 3, background=None)
    with pytest.raises(ValueError, match="cannot be held"):
        remove_small_components(t, 3, fill=256)
    with pytest.raises(TypeError, match="min_area"):
        remove_small_components(t, 2.5)
    with pytest.raises(ValueError, match="out must be"):
        remove_small_components(t, 3, out=torch.zeros((4, 5), dtype=torch.int16))
    huge = torch.zeros(1, dtype=torch.uint8).expand(1 << 16, 1 << 15)            # 2^31 positions, one byte of memory
    with pytest.raises(ValueError, match=r"2\^31 - 2"):
        connected_components(huge)
    with pytest.raises(ValueError, match=r"2\^31 - 2"):
        remove_small_components(huge, 3)
    cc, count = connected_components(torch.zeros((2, 4, 5), dtype=torch.uint8))
    with pytest.raises(ValueError, match="loop over the entries"):
        component_stats(cc, count)
    with pytest.raises(ValueError, match="loop over the entries"):
        component_stats(cc[None], None)
    with pytest.raises(TypeError, match="int32"):
        component_stats(cc.long())
    with pytest.raises(ValueError, match="does not match"):
        component_stats(cc[0], values=torch.zeros((4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="max_components"):
        component_stats(cc[0], max_components=-1)


def test_empty_inputs():
    cc, count = connected_components(torch.zeros((3, 0, 5), dtype=torch.int16))
    assert cc.shape == (3, 0, 5) and cc.dtype == torch.int32 and count.tolist() == [0, 0, 0]
    assert remove_small_components(torch.zeros((0, 5), dtype=torch.uint8), 3).shape == (0, 5)
    got = component_stats(torch.zeros((3, 4), dtype=torch.int32), values=torch.zeros((3, 4), dtype=torch.int16))
    assert got["area"].shape == (0,) and got["bbox"].shape == (0, 4) and got["value"].dtype == torch.int16


# ---------------------------------------------------------------------------------------------------------------- native, host only
def _plan(lib, dims, B, D, H, W):
    tile = (ctypes.c_int * 3)()
    tiles, chunks, label, remove = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    levels = ctypes.c_int()
    rc = lib.ptb_cc_plan(dims, B, D, H, W, tile, ctypes.byref(tiles), ctypes.byref(chunks), ctypes.byref(levels), ctypes.byref(label), ctypes.byref(remove))
    return rc, tuple(tile), tiles.value, chunks.value, levels.value, label.value, remove.value


def _up16(v):
    return (v + 15) // 16 * 16


def test_plan_geometry_and_workspace_over_a_sweep_of_extents():
    lib = N.load()
    extents = [(2, 1, 1, 1, 1), (2, 1, 1, 16, 64), (2, 3, 1, 17, 65), (2, 1, 1, 5000, 5000), (2, 7, 1, 1, 3000), (2, 2049, 1, 33, 31), (2, 1, 1, 46340, 46340),
               (3, 1, 4, 8, 32), (3, 2, 5, 9, 33), (3, 1, 512, 512, 512), (3, 4, 9, 17, 23), (3, 1, 1, 1, 1), (2, 5_000_000, 1, 1, 1)]
    for dims, B, D, H, W in extents:
        rc, tile, tiles, chunks, levels, label, remove = _plan(lib, dims, B, D, H, W)
        assert rc == 0, (dims, B, D, H, W)
        assert tile == ((1,) + C.TILE_2D if dims == 2 else C.TILE_3D) and tile[0] * tile[1] * tile[2] == 1024
        n = D * H * W
        assert tiles == B * -(-D // tile[0]) * -(-H // tile[1]) * -(-W // tile[2]) and tiles * 1024 >= B * n
        assert chunks == B * -(-n // 1024)
        m, cnt = chunks + 1, []
        while m > 2048:
            m = -(-m // 2048)
            cnt.append(m)
        assert levels == len(cnt) <= 4
        # every phase: the error words, the parent map, then either the second map (remove_small) or the counts, their scan and its sums
        head = _up16(4 * B) + _up16(4 * B * n)
        assert remove == head + _up16(4 * B * n)
        assert label == head + _up16(4 * (chunks + 1)) + _up16(8 * (chunks + 1)) + sum(_up16(8 * c) for c in cnt)
    assert lib.ptb_cc_plan(2, 1, 1, 4, 4, None, None, None, None, None, None) == 0


def test_entry_points_refuse_bad_arguments_without_a_device():
    """The entry points validate before they touch the device, so these calls are safe without a GPU."""
    lib = N.load()
    assert _plan(lib, 4, 1, 1, 4, 4)[0] == -1 and _plan(lib, 2, 1, 2, 4, 4)[0] == -1 and _plan(lib, 2, 0, 1, 4, 4)[0] == -1 and _plan(lib, 3, 1, 4, 0, 4)[0] == -1
    assert _plan(lib, 2, 1, 1, 1 << 16, 1 << 15)[0] == N.PTB_EUNSUPPORTED and _plan(lib, 3, 2, 1 << 10, 1 << 10, 1 << 10)[0] == N.PTB_EUNSUPPORTED
    assert _plan(lib, 2, 1, 1, 46341, 46341)[0] == N.PTB_EUNSUPPORTED
    fake = ctypes.c_void_p(4096)                      # (never dereferenced: every call below is refused first)
    odd = ctypes.c_void_p(4100)
    big = 1 << 40
    assert lib.ptb_cc_label(None, 1, 2, 1, 1, 4, 4, 8, 1, 0, fake, fake, fake, big, None) == -1
    assert lib.ptb_cc_label(fake, 3, 2, 1, 1, 4, 4, 8, 1, 0, fake, fake, fake, big, None) == -1            # element size
    assert lib.ptb_cc_label(fake, 1, 2, 1, 1, 4, 4, 6, 1, 0, fake, fake, fake, big, None) == -1            # connectivity of the other dims
    assert lib.ptb_cc_label(fake, 1, 3, 1, 4, 4, 4, 18, 1, 0, fake, fake, fake, big, None) == -1
    assert lib.ptb_cc_label(fake, 1, 1, 1, 1, 4, 4, 4, 1, 0, fake, fake, fake, big, None) == -1            # dims
    assert lib.ptb_cc_label(fake, 1, 2, 1, 1, 0, 4, 8, 1, 0, fake, fake, fake, big, None) == -1            # extents
    assert lib.ptb_cc_label(fake, 1, 2, 1, 1, 1 << 16, 1 << 15, 8, 1, 0, fake, fake, fake, big, None) == N.PTB_EUNSUPPORTED
    need = _plan(lib, 2, 1, 1, 4, 4)[5]
    assert lib.ptb_cc_label(fake, 1, 2, 1, 1, 4, 4, 8, 1, 0, fake, fake, fake, need - 1, None) == -1       # workspace too small
    assert lib.ptb_cc_label(fake, 1, 2, 1, 1, 4, 4, 8, 1, 0, fake, fake, odd, big, None) == -1             # ... or misaligned
    assert lib.ptb_cc_label(fake, 1, 2, 1, 1, 4, 4, 8, 1, 0, odd, fake, fake, big, None) == -1
    need = _plan(lib, 3, 2, 4, 4, 4)[6]
    assert lib.ptb_cc_remove_small(fake, 2, 3, 2, 4, 4, 4, 26, 1, 0, 5, 0, fake, fake, need - 1, None) == -1
    assert lib.ptb_cc_remove_small(fake, 2, 3, 2, 4, 4, 4, 8, 1, 0, 5, 0, fake, fake, big, None) == -1
    assert lib.ptb_cc_remove_small(fake, 5, 3, 2, 4, 4, 4, 26, 1, 0, 5, 0, fake, fake, big, None) == -1
    assert lib.ptb_cc_remove_small(fake, 2, 3, 2, 4, 4, 4, 26, 1, 0, 5, 0, None, fake, big, None) == -1
    assert lib.ptb_cc_stats(None, 2, 1, 4, 4, 3, None, 0, fake, fake, None, None) == -1
    assert lib.ptb_cc_stats(fake, 2, 1, 4, 4, 0, None, 0, fake, fake, None, None) == -1                    # no component to describe
    assert lib.ptb_cc_stats(fake, 2, 1, 4, 4, 3, fake, 1, fake, fake, None, None) == -1                    # values without a value row
    assert lib.ptb_cc_stats(fake, 2, 1, 4, 4, 3, fake, 3, fake, fake, fake, None) == -1
    assert lib.ptb_cc_stats(fake, 2, 2, 4, 4, 3, None, 0, fake, fake, None, None) == -1                    # a 2-D map has D = 1
