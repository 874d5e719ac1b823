"""CPU: how a band plan lays out the work items of a launch group for band_pair_kernel (csrc/ptb_bandpair.hip) -- first the pairs of
vertically adjacent full 64 x 64 items under the same covering tiles, then the items without a partner -- read through
ptb_band_plan_pairs.  Host-side planning only: no GPU needed.  The table itself (item count, bytes) is pinned by tests/test_plan_cpu.py."""
import ctypes

import numpy as np

from pytorch_toolbelt_amd import _native as N


def _pairs(shape, tile, step, rows=1024, C=3):
    """(item count of the plan, [(pair_cnt, single_cnt) per launch group]) of the slicer geometry."""
    from oracle import tiles_oracle as TO

    lib = N.load()
    geom = TO.slicer_geometry(shape, tile, step)
    xy = np.ascontiguousarray(np.asarray(geom["crops"], dtype=np.int64)[:, :2].T)
    H, W = geom["target_shape"]
    handle = ctypes.c_void_p()
    nbytes = lib.ptb_band_plan_create(xy[0].ctypes.data_as(N._i64p), xy[1].ctypes.data_as(N._i64p), xy.shape[1], C, tile, tile, H, W, rows, 0, H,
                                      None, 0, ctypes.byref(handle))
    assert nbytes > 0, nbytes
    try:
        ng, ni = ctypes.c_int(), ctypes.c_int64()
        assert lib.ptb_band_plan_info(handle, ctypes.byref(ng), None, ctypes.byref(ni), None, None) == 0
        groups = []
        for g in range(ng.value):
            pc, sc = ctypes.c_int(-1), ctypes.c_int(-1)
            assert lib.ptb_band_plan_pairs(handle, g, ctypes.byref(pc), ctypes.byref(sc)) == 0
            assert pc.value >= 0 and sc.value >= 0
            groups.append((pc.value, sc.value))
        assert lib.ptb_band_plan_pairs(handle, ng.value, None, None) == -1 and lib.ptb_band_plan_pairs(handle, -1, None, None) == -1
        assert lib.ptb_band_plan_pairs(None, 0, None, None) == -1
        assert nbytes == ni.value * 64
        return ni.value, groups
    finally:
        lib.ptb_band_plan_destroy(handle)


def test_every_item_of_the_headline_geometry_pairs():
    items, groups = _pairs((5000, 5000), 512, 256, C=4)
    assert len(groups) == 5 and items == (5120 // 64) * (5120 // 64)
    for pc, sc in groups:
        assert sc == 0 and 2 * pc == items // 5, (pc, sc)


def test_a_band_of_160_rows_is_a_pair_and_a_32_row_single_per_column():
    items, groups = _pairs((640, 640), 320, 160)
    assert items == (4 * 3) * (4 * 3)                         # four bands of 160 rows and four cells of 160 columns: 64, 64 and 32 each
    assert sum(2 * pc + sc for pc, sc in groups) == items
    assert sum(pc for pc, _ in groups) == sum(sc for _, sc in groups) == items // 3


def test_a_band_of_192_rows_is_a_pair_and_a_64_row_single_per_column():
    items, groups = _pairs((768, 768), 384, 192)
    assert sum(2 * pc + sc for pc, sc in groups) == items == 4 * (768 // 64) * 3
    assert sum(pc for pc, _ in groups) == sum(sc for _, sc in groups) == items // 3


def test_bands_of_one_item_row_have_no_pairs():
    items, groups = _pairs((256, 256), 128, 64)
    assert groups == [(0, items)]


def test_tile_rows_off_the_8_pixel_grid_have_no_pairs():
    """tile 256 / step 132: the second tile row starts at 132, the blocks of its tiles are not 16-byte aligned in a 16-bit plane."""
    items, groups = _pairs((520, 520), 256, 132)
    assert sum(sc for _, sc in groups) == items and all(pc == 0 for pc, _ in groups)


def test_plans_of_32_row_items_have_no_pairs():
    lib = N.load()
    assert lib.ptb_set_tunable(11, 32) == 0
    try:
        items, groups = _pairs((5000, 5000), 512, 256, C=4)
        assert items == (5120 // 64) * (5120 // 32)
        assert all(pc == 0 for pc, _ in groups) and sum(sc for _, sc in groups) == items
    finally:
        assert lib.ptb_set_tunable(11, 64) == 0


def test_the_pair_tunable_is_a_boolean_key():
    lib = N.load()
    try:
        for v in (0, 1, 7):
            assert lib.ptb_set_tunable(28, v) == 0
    finally:
        assert lib.ptb_set_tunable(28, 1) == 0
