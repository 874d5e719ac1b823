"""GPU: ``activation=`` / ``temperature=`` fused into mirror_volume_deaugment and the three VolumeMerger paths (ptb_volume_activation.hip)
against the float64 model of tests/volume_activation_cases.py (absolute 1e-5 on every value), bit for bit between the library's own paths,
exact saturation, and the errors."""
import pytest
import torch

import volume_activation_cases as VA
from volume_defer_cases import cases, wide_slab

pytestmark = pytest.mark.gpu

CASES = dict(cases(), wide_slab=wide_slab())
NAMES = sorted(CASES)
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
LAYOUTS = ["dense", "channels_last_3d"]
MIRRORS = ["w", "dh", "dhw"]
TEMPERATURE = 0.75      # z = x * t stays inside the [-3, 3] the tolerance was worked out for
# result kinds of the deferred merger: fp32 cdhw, fp32 dhwc, bf16, argmax uint8, argmax int64
KINDS = [dict(layout="cdhw", dtype=torch.float32, argmax=False), dict(layout="dhwc", dtype=torch.float32, argmax=False),
         dict(layout="cdhw", dtype=torch.bfloat16, argmax=False), dict(layout="cdhw", dtype=torch.uint8, argmax=True),
         dict(layout="dhwc", dtype=torch.int64, argmax=True)]


def _dev(y, layout="dense"):
    y = y.cuda()
    return y.contiguous(memory_format=torch.channels_last_3d) if layout == "channels_last_3d" else y


def _bits(t):
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16)
    return t


def _merger(case, channels, **kw):
    from pytorch_toolbelt_amd.inference.tiles_3d import VolumeMerger

    return VolumeMerger(case["shape"], channels, case["weight"], device="cuda", **kw)


def _feed(merger, fed, mirror, reduction, activation, temperature=TEMPERATURE):
    for y, rois in fed:
        if mirror is None:
            merger.integrate_batch(y, rois, activation=activation, temperature=temperature)
        else:
            merger.integrate_batch_deaugment(y, rois, mirror, reduction, activation=activation, temperature=temperature)


def _as_cdhw(out, kind):
    return out.permute(3, 0, 1, 2) if kind["layout"] == "dhwc" and not kind["argmax"] else out


# ------------------------------------------------------------------------------------------------ reduce
@pytest.mark.parametrize("activation, channels", [("softmax", c) for c in (1, 3, 4, 5, 8, 9, 16)] + [("sigmoid", c) for c in (3, 4, 20)])
def test_deaugment_matches_the_model(activation, channels):
    """Every source dtype and layout on a tile on the 4-voxel grid (4-voxel dense lanes up to 8 softmax channels, one-voxel lanes above;
    16- / 8-byte channels-last loads when C % 4 == 0) and on one off it; mirrors and reductions rotate."""
    from pytorch_toolbelt_amd import _native as N
    from pytorch_toolbelt_amd.inference.tta_3d import mirror_volume_deaugment

    i = 0
    for tile in ((6, 8, 12), (5, 6, 7)):
        for dtype in DTYPES:
            mirror = MIRRORS[(i + channels) % 3]
            reduction = VA.REDUCTIONS[(i // 2 + channels) % 3]
            y = VA.logits((2 ** len(mirror) * 2, channels) + tile, dtype, seed=10 * channels + i)      # B = 2
            want = VA.deaugment64(y, mirror, reduction, activation, TEMPERATURE)
            results = []
            for layout in LAYOUTS:
                before = N.calls
                got = mirror_volume_deaugment(_dev(y, layout), mirror, reduction, activation=activation, temperature=TEMPERATURE)
                assert N.calls == before + 1                    # one launch, no torch activation in front of it
                assert got.dtype == torch.float32 and got.is_contiguous()
                VA.assert_close(got, want, (activation, channels, tile, dtype, layout, mirror, reduction))
                results.append(got)
            assert torch.equal(results[0], results[1])          # dense == channels_last_3d, bit for bit
            i += 1


# ------------------------------------------------------------------------------------------------ accumulating merger
@pytest.mark.parametrize("name", ["half_overlap", "off_grid"])
@pytest.mark.parametrize("mirror", [None, "dhw"])
def test_accumulating_merger_matches_the_model(name, mirror):
    case = CASES[name]
    for i, (activation, reduction) in enumerate((("softmax", "mean"), ("sigmoid", "gmean"), ("softmax", "logodd"))):
        dtype, layout = DTYPES[i], LAYOUTS[i % 2]
        fed = VA.batches(case, 4, mirror, dtype, 5, seed=20 + i)
        want = VA.merge64(case, VA.model_tiles(fed, mirror, reduction, activation, TEMPERATURE))
        m = _merger(case, 4)
        _feed(m, [(_dev(y, layout), rois) for y, rois in fed], mirror, reduction, activation)
        VA.assert_close(m.merge(), want, (name, mirror, activation, reduction, dtype, layout))


def test_host_batch_is_uploaded_and_then_fused():
    case = CASES["off_grid"]
    fed = VA.batches(case, 3, None, torch.bfloat16, 4, seed=30)
    a, b = _merger(case, 3), _merger(case, 3)
    for y, rois in fed:
        a.integrate_batch(y, rois, activation="softmax")                    # CPU tensor
        b.integrate_batch(y.cuda(), rois, activation="softmax")
    a.accumulate_single(fed[0][0][0], fed[0][1][0], activation="sigmoid")
    b.accumulate_single(fed[0][0][0].cuda(), fed[0][1][0], activation="sigmoid")
    assert torch.equal(a.volume, b.volume) and torch.equal(a.norm_mask, b.norm_mask)


# ------------------------------------------------------------------------------------------------ deferred merger
@pytest.mark.parametrize("name", NAMES)
def test_deferred_merger_matches_the_model_and_the_accumulating_one(name):
    """All result kinds, with and without "dhw": against the float64 model, and bit for bit what the accumulating merger followed by
    merge_crop gives.  Source dtypes rotate over the cases, layouts and activations over the kinds."""
    case = CASES[name]
    ci = NAMES.index(name)
    channels = 4
    for mi, mirror in enumerate((None, "dhw")):
        dtype = DTYPES[(ci + mi) % 3]
        reduction = VA.REDUCTIONS[(ci + mi) % 3]
        fed = VA.batches(case, channels, mirror, dtype, 5, seed=40 + 2 * ci + mi)
        on_dev = {layout: [(_dev(y, layout), rois) for y, rois in fed] for layout in LAYOUTS}
        want = {}
        for ki, kind in enumerate(KINDS):
            activation = "sigmoid" if (ki + ci + mi) % 3 == 2 else "softmax"
            if activation not in want:
                want[activation] = VA.window_of(case, VA.merge64(case, VA.model_tiles(fed, mirror, reduction, activation, TEMPERATURE)))
            layout = LAYOUTS[(ki + mi) % 2]
            spec = dict(crop=case["window"], **kind)
            deferred, plain = _merger(case, channels, crops=case["crops"], defer=True, result=spec), _merger(case, channels)
            for m in (deferred, plain):
                _feed(m, on_dev[layout], mirror, reduction, activation)
            got = deferred.merge_crop(**spec)
            tag = (name, mirror, dtype, layout, activation, reduction, kind)
            assert len(deferred._held) == 0, tag
            assert torch.equal(_bits(got), _bits(plain.merge_crop(**spec))), tag         # deferred == accumulating + merge_crop
            if kind["argmax"]:
                VA.assert_argmax(got, want[activation], tag)
            elif kind["dtype"] == torch.float32:
                VA.assert_close(_as_cdhw(got, kind), want[activation], tag)
            else:
                VA.assert_half_close(_as_cdhw(got, kind), want[activation], tag)


# ------------------------------------------------------------------------------------------------ bit for bit between the library's paths
@pytest.mark.parametrize("activation, channels", [("softmax", 4), ("softmax", 6), ("softmax", 12), ("sigmoid", 20)])
def test_paths_agree_bit_for_bit(activation, channels):
    """dense == channels_last_3d, fused de-augmentation == integrate_batch(mirror_volume_deaugment(..)), 4-voxel / 16-byte lanes == the
    force-scalar ones -- in the accumulating and in the deferred merger."""
    from pytorch_toolbelt_amd import _native as N
    from pytorch_toolbelt_amd.inference.tta_3d import mirror_volume_deaugment

    case = CASES["half_overlap"]
    dtype = DTYPES[channels % 3]
    spec = dict(crop=case["window"], layout="cdhw", dtype=torch.float32, argmax=False)
    for mirror, reduction in ((None, "mean"), ("dhw", "gmean")):
        fed = VA.batches(case, channels, mirror, dtype, 4, seed=60 + channels)
        on_dev = {layout: [(_dev(y, layout), rois) for y, rois in fed] for layout in LAYOUTS}
        results = []
        try:
            for scalar in (0, 1):
                assert N.load().ptb_set_tunable(1, scalar) == 0
                for layout in LAYOUTS:
                    plain, deferred = _merger(case, channels), _merger(case, channels, crops=case["crops"], defer=True, result=spec)
                    _feed(plain, on_dev[layout], mirror, reduction, activation)
                    _feed(deferred, on_dev[layout], mirror, reduction, activation)
                    results += [plain.merge_crop(**spec), deferred.merge_crop(**spec)]
        finally:
            assert N.load().ptb_set_tunable(1, 0) == 0
        if mirror is not None:
            two_step = _merger(case, channels)
            for y, rois in on_dev["dense"]:
                p = mirror_volume_deaugment(y, mirror, reduction, activation=activation, temperature=TEMPERATURE)
                two_step.integrate_batch(p, rois)
            results.append(two_step.merge_crop(**spec))
        for r in results[1:]:
            assert torch.equal(_bits(r), _bits(results[0])), (activation, channels, mirror)


# ------------------------------------------------------------------------------------------------ saturation
@pytest.mark.parametrize("dtype, big", [(torch.float32, 100.0), (torch.float16, 65504.0)])
def test_saturated_logits_give_exact_probabilities(dtype, big):
    from pytorch_toolbelt_amd.inference.tta_3d import mirror_volume_deaugment

    case = CASES["half_overlap"]
    channels, n = 4, len(case["crops"])
    sign = torch.where(torch.rand((2 * n, channels) + case["tile"], generator=torch.Generator().manual_seed(1)) < 0.5, -1.0, 1.0)
    y = (sign * big).to(dtype)
    want = (sign > 0).float()
    for layout in LAYOUTS:
        got = mirror_volume_deaugment(_dev(y[:8], layout), "w", "mean", activation="sigmoid")
        # both views of a voxel: the mean of two exact 0 / 1 values
        assert torch.equal(got.cpu(), (want[:4] + want[4:8].flip(4)) / 2)
    # one channel at +big, the others at -big: softmax and sigmoid are both exactly one-hot
    hot = torch.randint(0, channels, (n,) + case["tile"], generator=torch.Generator().manual_seed(2))
    onehot = torch.nn.functional.one_hot(hot, channels).permute(0, 4, 1, 2, 3).float()
    z = ((onehot * 2 - 1) * big).to(dtype)
    for layout in LAYOUTS:
        got = mirror_volume_deaugment(_dev(z, layout), "w", "sum", activation="softmax")
        assert torch.isfinite(got).all() and torch.equal(got.cpu(), onehot[: n // 2] + onehot[n // 2:].flip(4))
    # ... and through the mergers, on tiles cut from one label volume: every tile over a voxel says the same exact 0 / 1, and so does the blend
    labels = torch.randint(0, channels, case["shape"], generator=torch.Generator().manual_seed(3))
    volume = torch.nn.functional.one_hot(labels, channels).permute(3, 0, 1, 2).float()
    tiles = torch.stack([volume[(slice(None),) + tuple(crop)] for crop in case["crops"]])
    z = ((tiles * 2 - 1) * big).to(dtype)
    spec = dict(crop=case["window"], layout="cdhw", dtype=torch.float32, argmax=False)
    for layout in LAYOUTS:
        batch = _dev(z, layout)
        for activation in ("softmax", "sigmoid"):
            plain, deferred = _merger(case, channels), _merger(case, channels, crops=case["crops"], defer=True, result=spec)
            for m in (plain, deferred):
                m.integrate_batch(batch, case["crops"], activation=activation)
            for out in (plain.merge_crop(**spec), deferred.merge_crop(**spec)):
                assert torch.equal(out.cpu(), VA.window_of(case, volume)), (layout, activation)


# ------------------------------------------------------------------------------------------------ errors
def test_softmax_channel_limit_and_one_activation_per_image():
    from pytorch_toolbelt_amd.inference.tta_3d import mirror_volume_deaugment

    case = CASES["single_tile"]
    y = torch.zeros((2, 17) + case["tile"], device="cuda")
    rois = case["crops"]
    with pytest.raises(NotImplementedError, match=r"y\.softmax\(1\)"):
        mirror_volume_deaugment(y, "w", "mean", activation="softmax")
    for m in (_merger(case, 17), _merger(case, 17, crops=rois, defer=True)):
        with pytest.raises(NotImplementedError, match=r"y\.softmax\(1\)"):
            m.integrate_batch(y[:1], rois, activation="softmax")
        with pytest.raises(NotImplementedError, match=r"y\.softmax\(1\)"):
            m.integrate_batch_deaugment(y, rois, "w", "mean", activation="softmax")
        m.integrate_batch(y[:1], rois, activation="sigmoid")           # sigmoid serves any C
    assert mirror_volume_deaugment(y, "w", "mean", activation="sigmoid").shape == (1, 17) + case["tile"]

    case = CASES["half_overlap"]
    fed = [(_dev(y), rois) for y, rois in VA.batches(case, 2, None, torch.float32, 2, seed=70)]
    m = _merger(case, 2, crops=case["crops"], defer=True)
    m.integrate_batch(*fed[0], activation="softmax")
    for kw in (dict(activation="sigmoid"), dict(activation="softmax", temperature=0.5), dict()):
        with pytest.raises(RuntimeError, match="activation"):
            m.integrate_batch(*fed[1], **kw)
    m.integrate_batch(*fed[1], activation="softmax")                    # the refused calls recorded nothing
    m.reset()
    _feed(m, fed, None, "mean", "sigmoid", 0.5)
    want = VA.window_of(case, VA.merge64(case, VA.model_tiles([(y.cpu(), r) for y, r in fed], None, "mean", "sigmoid", 0.5)))
    VA.assert_close(m.merge(), want, "after reset")
