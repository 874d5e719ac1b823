"""CPU: the host form of utils/instances.py equals the yardstick of instances_cases.py over the whole case list, the yardstick's table
equals sklearn's contingency matrix, the case list is not vacuous, and every validation error and the max_pairs contract hold."""
import numpy as np
import pytest
import torch

import instances_cases as IC
from pytorch_toolbelt_amd.utils import instance_overlaps, match_instances


def _maps(c):
    return torch.from_numpy(np.ascontiguousarray(c.pred)), torch.from_numpy(np.ascontiguousarray(c.truth))


def test_yardstick_table_is_sklearns_contingency_matrix():
    from sklearn.metrics.cluster import contingency_matrix

    for name in IC.names():
        c = IC.case(name)
        p, t = IC._clamp(c.pred, c.n_pred), IC._clamp(c.truth, c.n_truth)
        m = contingency_matrix(t, p, sparse=True).tocoo()
        ids_t, ids_p = np.unique(t), np.unique(p)
        want = {(int(ids_p[j]), int(ids_t[i])): int(v) for i, j, v in zip(m.row, m.col, m.data) if ids_p[j] > 0 and ids_t[i] > 0 and v}
        tab = IC.expected_table(name)
        got = {(int(a), int(b)): int(v) for (a, b), v in zip(tab["pairs"], tab["intersection"])}
        assert got == want, name
        assert len(got) == len(tab["pairs"]), name


def test_case_list_is_not_vacuous():
    plain = {name: IC.expected(name) for name in IC.names()}
    assert any(r["tp"][0] > 0 and r["fp"][0] > 0 and r["fn"][0] > 0 and r["tp"][0] != r["tp"][1] for r in plain.values())
    assert any(IC.expected(name, True)["rejected_for_class"] > 0 for name in IC.names())
    half, quarters = plain["iou_half"], plain["iou_three_quarters"]
    assert half["tp"].tolist() == [0, 0, 0] and half["num_pairs"] == 1                       # IoU is exactly 0.5: no match at 0.5
    assert quarters["tp"].tolist() == [1, 0, 0] and quarters["pred_iou"][0] == 0.75          # exactly 0.75: a match at 0.5, none at 0.75
    assert plain["noise"]["num_pairs"] > 2000 and plain["giant"]["num_pairs"] == 1024
    assert len(IC.expected_table("long_run")["pairs"]) == 3 and IC.expected_table("long_run")["intersection"].max() > 4096


@pytest.mark.parametrize("name", IC.names())
def test_host_form_equals_yardstick(name):
    c = IC.case(name)
    p, t = _maps(c)
    got = instance_overlaps(p, t, c.n_pred, c.n_truth)
    want = IC.expected_table(name)
    for key in ("pairs", "intersection", "pred_area", "truth_area"):
        assert got[key].numpy().dtype == want[key].dtype and np.array_equal(got[key].numpy(), want[key]), (name, key)
    assert got["num_pairs"].dim() == 0 and int(got["num_pairs"]) == len(want["pairs"])
    for thresholds in ((0.5,), IC.THRESHOLDS):
        IC.assert_matches(match_instances(p, t, thresholds, c.n_pred, c.n_truth), IC.expected(name, False, thresholds), c.n_pred, (name, thresholds))
        got = match_instances(p, t, thresholds, c.n_pred, c.n_truth, pred_class=torch.from_numpy(c.class_pred), truth_class=torch.from_numpy(c.class_truth),
                              num_classes=IC.NUM_CLASSES)
        assert got["tp"].shape == (IC.NUM_CLASSES, len(thresholds)) and got["pq"].shape == (IC.NUM_CLASSES, len(thresholds))
        IC.assert_matches(got, IC.expected(name, True, thresholds), c.n_pred, (name, thresholds, "classes"))


def test_counts_from_tensors_and_from_the_maps():
    c = IC.case("blobs")
    p, t = _maps(c)
    want = IC.expected("blobs")
    IC.assert_matches(match_instances(p, t, IC.THRESHOLDS), want, c.n_pred, "max")
    IC.assert_matches(match_instances(p, t, IC.THRESHOLDS, torch.tensor(c.n_pred), torch.tensor(c.n_truth)), want, c.n_pred, "0-dim")
    assert match_instances(p, t, 0.5)["tp"].shape == (1,)


def test_classes_outside_the_range_count_nowhere():
    c = IC.case("blobs")
    p, t = _maps(c)
    got = match_instances(p, t, IC.THRESHOLDS, c.n_pred, c.n_truth, pred_class=torch.from_numpy(c.class_pred).to(torch.uint8),
                          truth_class=torch.from_numpy(c.class_truth).to(torch.int16), num_classes=3)
    want = IC.match(c.pred, c.truth, c.n_pred, c.n_truth, IC.THRESHOLDS, c.class_pred, c.class_truth, 3)
    assert (c.class_pred >= 3).any()
    IC.assert_matches(got, want, c.n_pred, "K = 3")
    assert int((got["tp"] + got["fp"]).sum(0)[0]) == int((c.class_pred < 3).sum())


def test_max_pairs_contract():
    for name in ("blobs", "noise", "small"):
        c = IC.case(name)
        p, t = _maps(c)
        tab = IC.expected_table(name)
        P = len(tab["pairs"])
        got = instance_overlaps(p, t, c.n_pred, c.n_truth, max_pairs=P + 3)
        assert got["pairs"].shape == (P + 3, 2) and int(got["num_pairs"]) == P
        assert np.array_equal(got["pairs"][:P].numpy(), tab["pairs"]) and not got["pairs"][P:].any() and not got["intersection"][P:].any()
        assert int(instance_overlaps(p, t, c.n_pred, c.n_truth, max_pairs=P)["num_pairs"]) == P
        assert int(instance_overlaps(p, t, c.n_pred, c.n_truth, max_pairs=P - 1)["num_pairs"]) == -1
        IC.assert_matches(match_instances(p, t, IC.THRESHOLDS, c.n_pred, c.n_truth, max_pairs=P), IC.expected(name), c.n_pred, name)
        over = match_instances(p, t, IC.THRESHOLDS, c.n_pred, c.n_truth, max_pairs=P - 1)
        assert int(over["num_pairs"]) == -1
        for key in ("sq", "rq", "pq", "ap"):
            assert torch.isnan(over[key]).all(), key


def test_empty_inputs():
    e = torch.zeros((0, 5), dtype=torch.int32)
    got = instance_overlaps(e, e)
    assert got["pairs"].shape == (0, 2) and got["pred_area"].shape == (0,) and int(got["num_pairs"]) == 0
    assert instance_overlaps(e, e, 3, 2, max_pairs=4)["pairs"].shape == (4, 2)
    got = match_instances(e, e, (0.5, 0.75), 3, 2)
    assert got["pred_match"].shape == (3,) and got["truth_iou"].shape == (2,) and got["tp"].tolist() == [0, 0] and torch.isnan(got["pq"]).all()


def test_validation_errors():
    c = IC.case("small")
    p, t = _maps(c)
    with pytest.raises(TypeError):
        instance_overlaps(p.long(), t)
    with pytest.raises(TypeError):
        match_instances(p.numpy(), t)
    with pytest.raises(ValueError, match="same shape"):
        instance_overlaps(p, t[:, :4])
    with pytest.raises(ValueError, match="same device"):
        match_instances(p, t.to("meta"))
    with pytest.raises(ValueError, match="2\\^31 - 2"):
        big = torch.empty((1 << 16, 1 << 15), dtype=torch.int32, device="meta")
        instance_overlaps(big, big, 1, 1)
    with pytest.raises(ValueError, match="num_pred"):
        instance_overlaps(p, t, -1, 2)
    with pytest.raises(ValueError, match="0-dim"):
        instance_overlaps(p, t, torch.tensor([3]), 2)
    with pytest.raises(TypeError):
        instance_overlaps(p, t, 3.0, 2)
    with pytest.raises(ValueError, match="max_pairs"):
        instance_overlaps(p, t, max_pairs=-1)
    with pytest.raises(ValueError, match="max_pairs"):
        instance_overlaps(p, t, max_pairs=(1 << 28) + 1)
    for bad in ((0.4,), (0.5, 1.0), (0.75, 0.5), (0.5, 0.5), (), tuple([0.5 + 0.01 * i for i in range(17)]), (float("nan"),)):
        with pytest.raises(ValueError, match="threshold"):
            match_instances(p, t, bad)
    with pytest.raises(TypeError):
        match_instances(p, t, "x")
    cp, ct = torch.from_numpy(c.class_pred), torch.from_numpy(c.class_truth)
    for kwargs in (dict(pred_class=cp), dict(pred_class=cp, truth_class=ct), dict(num_classes=3), dict(truth_class=ct, num_classes=3)):
        with pytest.raises(ValueError, match="together"):
            match_instances(p, t, **kwargs)
    with pytest.raises(ValueError, match="shape"):
        match_instances(p, t, pred_class=cp[:-1], truth_class=ct, num_classes=3)
    with pytest.raises(TypeError):
        match_instances(p, t, pred_class=cp.double(), truth_class=ct, num_classes=3)
    with pytest.raises(ValueError, match="num_classes"):
        match_instances(p, t, pred_class=cp, truth_class=ct, num_classes=0)


def test_plan_states_its_workspace():
    """the formula of DESIGN.md ("Instance matching"), host only"""
    import ctypes

    from pytorch_toolbelt_amd import _native as N

    lib = N.load()

    def up16(v):
        return (v + 15) & ~15

    def plan(n, n_p, n_t, m, T, K):
        slots, ws, out = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        offs = (ctypes.c_int64 * 17)()
        assert lib.ptb_inst_plan(n, n_p, n_t, m, T, K, ctypes.byref(slots), ctypes.byref(ws), offs, ctypes.byref(out)) == 0
        return slots.value, ws.value, list(offs), out.value

    slots, ws, offs, out = plan(120000, 300, 280, 1000, 0, 0)
    words = (120000 + 31) // 32
    assert slots == 2048 and all(o % 16 == 0 for o in offs) and offs == sorted(offs)
    assert ws == 16 + up16(8 * slots) + 2 * up16(4 * slots) + up16(4 * words) + up16(4 * (words + 1)) + up16(8 * (words + 1)) + up16(8 * 2)
    assert out == 16 + up16(8 * 300) + up16(8 * 280) + up16(8 * 1000) + up16(8 * 1000)
    slots, ws, offs, out = plan(120000, 3000, 280, 1000, 3, 5)
    assert ws == 16 + up16(8 * slots) + 2 * up16(4 * slots) + up16(4 * 3 * 15) + up16(8 * 3 * 15) + up16(4 * 3 * 5) + up16(4 * 1 * 5)
    assert plan(10, 1, 1, 0, 0, 0)[0] == 2 and plan(10, 1, 1, 3, 1, 0)[0] == 8
    assert lib.ptb_inst_plan(1 << 31, 1, 1, 1, 0, 0, None, None, None, None) == N.PTB_EUNSUPPORTED
    assert lib.ptb_inst_plan(10, 1, 1, 1, 17, 0, None, None, None, None) == -1
    assert lib.ptb_inst_overlaps(None, None, 10, 1, 1, 1, None, 0, None, 0, None) == -1
