"""GPU: the instance-matching kernels (csrc/ptb_instances.hip) equal the yardstick of tests/instances_cases.py over the whole case list:
the overlap table, its row order, areas, matches and the float64 IoUs bit for bit, the IoU sums and scores within the bound of a
double sum.  The overflow paths (max_pairs below the number of distinct pairs, a table of 16 slots under thousands of pairs) are
ordinary error paths: they return num_pairs == -1."""
import numpy as np
import pytest
import torch

import instances_cases as IC
from pytorch_toolbelt_amd import _native as N
from pytorch_toolbelt_amd.utils import component_stats, connected_components, instance_overlaps, match_instances

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _dev(a, offset=False):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if offset:                                       # a contiguous view that starts one element into its buffer: the peeled loads
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        return view
    return t.to(DEV)


def _maps(c):
    return _dev(c.pred, c.offset), _dev(c.truth, c.offset)


def _classes(c):
    return dict(pred_class=torch.from_numpy(c.class_pred).to(DEV), truth_class=torch.from_numpy(c.class_truth).to(DEV), num_classes=IC.NUM_CLASSES)


def _once(f, *args, **kwargs):
    before = N.calls
    res = f(*args, **kwargs)
    assert N.calls == before + 1, "one native call per public call"
    assert all(v.device == DEV for v in res.values())
    return res


@pytest.mark.parametrize("name", IC.names())
def test_overlap_table_in_first_position_order(name):
    c = IC.case(name)
    p, t = _maps(c)
    want = IC.expected_table(name)
    got = _once(instance_overlaps, p, t, c.n_pred, c.n_truth)
    for key in ("pairs", "intersection", "pred_area", "truth_area"):
        g = got[key].cpu().numpy()
        assert g.dtype == want[key].dtype and g.shape == want[key].shape and np.array_equal(g, want[key]), (name, key)
    assert got["num_pairs"].dim() == 0 and got["num_pairs"].dtype == torch.int64 and int(got["num_pairs"]) == len(want["pairs"])


@pytest.mark.parametrize("name", IC.names())
def test_matching_equals_yardstick(name):
    c = IC.case(name)
    p, t = _maps(c)
    for thresholds in ((0.5,), IC.THRESHOLDS):
        got = _once(match_instances, p, t, thresholds, c.n_pred, c.n_truth)
        IC.assert_matches(got, IC.expected(name, False, thresholds), c.n_pred, (name, thresholds))
        got = _once(match_instances, p, t, thresholds, c.n_pred, c.n_truth, **_classes(c))
        IC.assert_matches(got, IC.expected(name, True, thresholds), c.n_pred, (name, thresholds, "classes"))


def test_counts_read_back_and_class_dtypes():
    c = IC.case("blobs")
    p, t = _maps(c)
    want = IC.expected("blobs", True)
    kw = _classes(c)
    kw["pred_class"], kw["truth_class"] = kw["pred_class"].to(torch.uint8), kw["truth_class"].to(torch.int16)
    IC.assert_matches(match_instances(p, t, IC.THRESHOLDS, **kw), want, c.n_pred, "max, uint8 / int16 classes")
    counts = torch.tensor(c.n_pred, device=DEV), torch.tensor(c.n_truth, device=DEV)
    IC.assert_matches(match_instances(p, t, IC.THRESHOLDS, *counts), IC.expected("blobs"), c.n_pred, "0-dim counts")
    got = match_instances(p, t, IC.THRESHOLDS, c.n_pred, c.n_truth, pred_class=kw["pred_class"], truth_class=kw["truth_class"], num_classes=3)
    IC.assert_matches(got, IC.match(c.pred, c.truth, c.n_pred, c.n_truth, IC.THRESHOLDS, c.class_pred, c.class_truth, 3), c.n_pred, "K = 3")


@pytest.mark.parametrize("name", ["noise", "giant"])
def test_two_runs_are_bit_identical(name):
    c = IC.case(name)
    p, t = _maps(c)
    first = match_instances(p, t, IC.THRESHOLDS, c.n_pred, c.n_truth, **_classes(c))
    table = instance_overlaps(p, t, c.n_pred, c.n_truth)
    for _ in range(2):
        again = match_instances(p, t, IC.THRESHOLDS, c.n_pred, c.n_truth, **_classes(c))
        for key, v in first.items():
            assert torch.equal(v.view(torch.int64) if v.dtype == torch.float64 else v, again[key].view(torch.int64) if v.dtype == torch.float64 else again[key]), key
        for key, v in instance_overlaps(p, t, c.n_pred, c.n_truth).items():
            assert torch.equal(v, table[key]), key


@pytest.mark.parametrize("name", ["noise", "blobs", "small"])
def test_max_pairs_contract(name):
    c = IC.case(name)
    p, t = _maps(c)
    tab = IC.expected_table(name)
    P = len(tab["pairs"])
    before = N.calls
    got = instance_overlaps(p, t, c.n_pred, c.n_truth, max_pairs=P + 3)
    assert N.calls == before + 1
    assert got["pairs"].shape == (P + 3, 2) and got["intersection"].shape == (P + 3,) and int(got["num_pairs"]) == P
    assert np.array_equal(got["pairs"][:P].cpu().numpy(), tab["pairs"]) and np.array_equal(got["intersection"][:P].cpu().numpy(), tab["intersection"])
    assert not got["pairs"][P:].any() and not got["intersection"][P:].any()
    exact = instance_overlaps(p, t, c.n_pred, c.n_truth, max_pairs=P)
    assert int(exact["num_pairs"]) == P and np.array_equal(exact["pairs"].cpu().numpy(), tab["pairs"])
    IC.assert_matches(match_instances(p, t, IC.THRESHOLDS, c.n_pred, c.n_truth, max_pairs=P), IC.expected(name), c.n_pred, (name, "P"))
    for m in sorted({P - 1, min(8, P - 1), 0}):     # one row short; a table of 16 slots under thousands of pairs; no row at all
        over = instance_overlaps(p, t, c.n_pred, c.n_truth, max_pairs=m)
        assert int(over["num_pairs"]) == -1 and over["pairs"].shape == (m, 2), (name, m)
        over = match_instances(p, t, IC.THRESHOLDS, c.n_pred, c.n_truth, max_pairs=m)
        assert int(over["num_pairs"]) == -1, (name, m)
        for key in ("sq", "rq", "pq", "ap"):
            assert torch.isnan(over[key]).all(), (name, m, key)
    torch.cuda.synchronize()


def test_non_default_stream_and_non_contiguous_inputs():
    c = IC.case("blobs_big")
    want = IC.expected("blobs_big")
    p, t = _maps(c)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        got = _once(match_instances, p, t, IC.THRESHOLDS, c.n_pred, c.n_truth)
        table = _once(instance_overlaps, p, t, c.n_pred, c.n_truth, max_pairs=4096)
    stream.synchronize()
    IC.assert_matches(got, want, c.n_pred, "stream")
    P = int(table["num_pairs"])
    assert np.array_equal(table["pairs"][:P].cpu().numpy(), IC.expected_table("blobs_big")["pairs"])
    pt, tt = _dev(np.ascontiguousarray(c.pred.T)).T, _dev(np.ascontiguousarray(c.truth.T)).T       # the same maps with transposed strides
    assert not pt.is_contiguous() and pt.shape == p.shape
    IC.assert_matches(_once(match_instances, pt, tt, IC.THRESHOLDS, c.n_pred, c.n_truth), want, c.n_pred, "strides")
    wide_p, wide_t = torch.zeros((300, 800), dtype=torch.int32, device=DEV), torch.zeros((300, 800), dtype=torch.int32, device=DEV)
    wide_p[:, ::2], wide_t[:, ::2] = p, t
    got = _once(instance_overlaps, wide_p[:, ::2], wide_t[:, ::2], c.n_pred, c.n_truth)
    assert np.array_equal(got["pairs"].cpu().numpy(), IC.expected_table("blobs_big")["pairs"])


def test_empty_inputs_launch_nothing():
    e = torch.zeros((0, 7), dtype=torch.int32, device=DEV)
    before = N.calls
    got = instance_overlaps(e, e, 3, 2)
    assert got["pairs"].shape == (0, 2) and got["pred_area"].tolist() == [0, 0, 0] and got["pairs"].device == DEV
    got = match_instances(e, e, (0.5, 0.75), 3, 2)
    assert got["tp"].tolist() == [0, 0] and torch.isnan(got["ap"]).all() and got["pred_match"].shape == (3,)
    assert N.calls == before


def test_chain_from_label_maps():
    """connected_components of two label maps -> component_stats(values=) -> match_instances with classes: equals the yardstick fed with the
    flood fill's maps"""
    a, b = IC.chain_labels()
    c = IC.case("blobs")
    la, lb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    cc_p, n_p = connected_components(la, connectivity=8)
    cc_t, n_t = connected_components(lb, connectivity=8)
    assert int(n_p) == c.n_pred and int(n_t) == c.n_truth
    cls_p = component_stats(cc_p, n_p, values=la)["value"]
    cls_t = component_stats(cc_t, n_t, values=lb)["value"]
    got = _once(match_instances, cc_p, cc_t, IC.THRESHOLDS, n_p, n_t, pred_class=cls_p, truth_class=cls_t, num_classes=IC.NUM_CLASSES)
    IC.assert_matches(got, IC.expected("blobs", True), c.n_pred, "chain")
