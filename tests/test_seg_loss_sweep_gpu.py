"""GPU half of the sweep of csrc/ptb_losses.hip (tests/test_seg_loss_sweep_cpu.py is the other half): every case of
tests/seg_loss_cases.py through its autograd Function of losses/_kernels.py, against the float64 model of oracle/seg_loss_oracle.py.

Per case, with no element of any comparison masked out:
* T_c of hard labels and 0 / 1 targets equal to the model exactly; the focal sums, the normaliser sums, I_c, P_c, the element-wise and
  per-pixel maps, the scalar loss and its coefficients within rtol = atol = 1e-5 (sums: atol * max(1, |model|));
* the gradient against float64 autograd of the reference's chain with seeded unit-scale upstream coefficients: rtol 2e-4, atol 2e-6 on
  tame pixels, atol 1e-4 on extreme ones (which pixels are extreme is decided from the logits);
* a second identical call returns the same bits; after a one-launch call the workspace of ``region_workspace`` is all zero;
* the C entry points that were really called, and their return codes, are the ones the restated dispatch predicts
  (``seg_loss_cases.entry_points``): where ptb_region_loss_fwd / ptb_seg_fused_bwd decline, the fall-back is the predicted one.
One more case per forward arm that reads labels carries a label outside [0, C): the sums finalise to NaN, ``flush_label_check()``
raises, the next clean call is finite.  And one child process runs every case once under the HIP runtime's launch log
(AMD_LOG_LEVEL=3 names each kernel it dispatches): the instances that really ran are the ones ``forward_arm`` / ``backward_arm`` name,
so a change of the real dispatch -- or a wrong restatement -- fails here.

Worst error / tolerance per family (values, gradients): the HIP kernels on MI355X | the float32 reference chain on the CPU
    SigmoidFocalSums  0.021, 0.067  | 0.022, 0.072        FocalScalar  0.0031, 0.0058 | 0.0069, 0.0058
    RegionStats       0.0071, 0.18  | 0.009, 0.17         RegionLoss   0.01, 0.069    | 0.011, 0.072
    SoftmaxFocalSums  0.077, 0.23   | 0.063, 0.23         FusedSegSums 0.0066, 0.18   | 0.0097, 0.2
    module            0.0069, 0.16  | 0.0061, 0.1"""
import contextlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import seg_loss_cases as SC

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nHIP kernels, worst error / tolerance (values, gradients): " + ", ".join("%s %.2g, %.2g" % (k, v[0], v[1]) for k, v in sorted(WORST.items())))


def _note(family, values, grads):
    old = WORST.get(family, (0.0, 0.0))
    WORST[family] = (max(old[0], values), max(old[1], grads))


def _K():
    from pytorch_toolbelt_amd.losses import _kernels as K

    return K


class _Spy:
    """The loaded library with a log of the entry points called and what each returned."""

    def __init__(self, lib):
        self._lib, self.log = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            rc = fn(*args)
            self.log.append("%s:%d" % (name, rc) if isinstance(rc, int) and name != "ptb_region_workspace_bytes" else name)
            return rc

        return call


@contextlib.contextmanager
def _configured(case):
    """The tunables and the one-launch switch of a case, restored afterwards; the library's entry points under a spy."""
    K = _K()
    N = K.N
    lib = N.load()
    spy = _Spy(lib)
    real_load, one_launch = N.load, K.ONE_LAUNCH_REGION_LOSS
    try:
        for key, value in zip(SC.TUN_KEYS, case.tun):
            assert lib.ptb_set_tunable(key, value) == 0
        K.ONE_LAUNCH_REGION_LOSS = case.one_launch
        N.load = lambda: spy
        yield spy
    finally:
        N.load = real_load
        K.ONE_LAUNCH_REGION_LOSS = one_launch
        for key, value in zip(SC.TUN_KEYS, SC.DEFAULT_TUN):
            lib.ptb_set_tunable(key, value)


def _place(a, off, dev):
    """``a`` on the device, ``off`` elements into an allocation that starts on the 16-byte grid."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + off * t.element_size()
    return view


def _tensors(case, inp, dev, labels=None):
    ox, ol, od = case.off
    x = _place(inp["x"], ox, dev).requires_grad_(True)
    return x, _place(inp["labels"] if labels is None else labels, ol, dev), _place(inp["dense"], od, dev), _place(inp["cw"], 0, dev)


def _call(case, x, labels, dense, cw, dev):
    """{key: tensor} of what the Function of a case returns (None: FocalScalar declined), keys as in ``seg_loss_cases.model``."""
    K = _K()
    f, ign = SC.flags_of(case), case.ignore
    il = int(ign) if (ign is not None and labels is not None) else 0
    iv = float(ign) if ign is not None else 0.0
    alpha, thr = float(case.alpha or 0.0), float(case.threshold or 0.0)
    fam = case.family
    if fam == "SigmoidFocalSums":
        sums, elem = K.SigmoidFocalSums.apply(x, labels, dense, cw, f, case.gamma, alpha, thr, il, iv)
        return dict(focal=sums, elem=elem) if case.elem else dict(focal=sums)
    if fam == "FocalScalar":
        loss = K.FocalScalar.run(x, labels, f, case.gamma, 1.0 / SC.numel(case))
        return None if loss is None else dict(loss=loss)
    if fam == "RegionStats":
        return dict(stats=K.RegionStats.apply(x, labels, dense, case.prob, ign is not None, il, iv))
    if fam == "SoftmaxFocalSums":
        sums, pix = K.SoftmaxFocalSums.apply(x, labels, cw, 1 if case.threshold is not None else 0, case.gamma, thr, int(ign), case.elem)
        return dict(focal=sums, elem=pix) if case.elem else dict(focal=sums)
    if fam == "FusedSegSums":
        focal, stats = K.FusedSegSums.apply(x, labels, dense, cw, f, case.prob, case.gamma, alpha, thr, il, iv)
        return dict(focal=focal, stats=stats)
    assert fam == "RegionLoss"
    e = SC.epilogue_kwargs(case)
    mask = None if e["class_mask"] is None else torch.from_numpy(e["class_mask"]).to(dev)
    loss = K.RegionLoss.apply(x, labels, dense, cw, f, case.prob, case.gamma, alpha, thr, il, iv, case.epi.with_focal, e["focal_scale"], e["dice_weight"],
                              e["jaccard_weight"], e["smooth"], e["eps"], e["log_loss"], mask, e["n_selected"])
    return dict(loss=loss, coef=loss.grad_fn.saved_tensors[4])


def _one_launch(case):
    return (case.family == "RegionLoss" and case.one_launch) or (case.family == "FocalScalar" and SC.forward_arm(case) != "unsupported")


def _workspace_is_zero(case, dev):
    """Every workspace ``region_workspace`` has handed out (read from its cache: asking again would go through the library)."""
    torch.cuda.synchronize(dev)
    held = list(_K()._workspaces.values())
    return bool(held) and not any(bool(ws.any()) for ws in held)


def _backward(out, up):
    total = None
    for k, v in out.items():
        if k != "coef":
            term = (v * torch.from_numpy(np.asarray(up[k])).to(device=v.device, dtype=v.dtype)).sum().double()
            total = term if total is None else total + term
    total.backward()


@pytest.mark.parametrize("case", SC.FUNCTIONS, ids=SC.ids)
def test_function_against_the_float64_model(case, dev):
    K = _K()
    N = K.N
    inp = SC.inputs(case)
    up = SC.upstream(case, inp)
    x, labels, dense, cw = _tensors(case, inp, dev)
    with _configured(case) as spy:
        before = N.calls
        out = _call(case, x, labels, dense, cw, dev)
        if out is None:
            assert SC.forward_arm(case) == "unsupported" and spy.log == SC.entry_points(case) and N.calls == before
            return
        assert SC.forward_arm(case) != "unsupported"
        if _one_launch(case):
            assert _workspace_is_zero(case, dev)
        _backward(out, up)
        assert N.calls > before
        assert spy.log == SC.entry_points(case), (spy.log, SC.forward_arm(case), SC.backward_arm(case))
        again = _call(case, x, labels, dense, cw, dev)
        for k in out:
            assert torch.equal(out[k], again[k]), "a second identical call differs in " + k
        if _one_launch(case):
            assert _workspace_is_zero(case, dev)
    K.flush_label_check()
    got = {k: v.detach().cpu().numpy() for k, v in out.items()}
    want = SC.model(case, inp)
    assert sorted(got) == sorted(want)
    ratios = SC.value_ratios(case, got, want)
    _out64, grad64 = SC.chain_gradient(case, torch.float64, inp, up)
    rg = SC.gradient_ratio(x.grad.cpu().numpy(), grad64, inp["x"])
    _note(case.family, max(ratios.values()), rg)
    print("%s: forward %s, backward %s, values %s, gradient %.3g" % (case.name, SC.forward_arm(case), SC.backward_arm(case),
                                                                    ", ".join("%s %.3g" % kv for kv in sorted(ratios.items())), rg))
    assert all(r <= 1.0 for r in ratios.values()), ratios
    assert rg <= 1.0, rg


@pytest.mark.parametrize("case", SC.bad_label_cases(), ids=SC.ids)
def test_label_outside_the_classes_poisons_the_sums(case, dev):
    K = _K()
    inp = SC.inputs(case)
    K.flush_label_check()
    x, labels, dense, cw = _tensors(case, inp, dev, labels=SC.bad_labels(case, inp))
    with _configured(case):
        out = _call(case, x, labels, dense, cw, dev)
        for k, v in out.items():
            if k in ("focal", "stats", "loss"):
                assert torch.isnan(v).all(), k
        with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes"):
            K.flush_label_check()
        if _one_launch(case):
            assert _workspace_is_zero(case, dev)
        x, labels, dense, cw = _tensors(case, inp, dev)
        out = _call(case, x, labels, dense, cw, dev)
        for k, v in out.items():
            assert torch.isfinite(v).all(), k
        K.flush_label_check()
        want = SC.model(case, inp)
        ratios = SC.value_ratios(case, {k: v.detach().cpu().numpy() for k, v in out.items()}, want)
        assert all(r <= 1.0 for r in ratios.values()), ratios


def _module(case):
    from pytorch_toolbelt_amd import losses as L

    cls, kw = case.module
    kw = dict(kw)
    mode = "multiclass" if case.target == "labels" else "multilabel"
    if cls in ("BinaryFocalLoss", "CrossEntropyFocalLoss"):
        return getattr(L, cls)(**kw)
    return getattr(L, cls)(mode, **kw)


@pytest.mark.parametrize("case", SC.MODULES, ids=SC.ids)
def test_public_classes_route_to_the_functions(case, dev):
    """BinaryFocalLoss, CrossEntropyFocalLoss, DiceLoss, JaccardLoss and FocalDiceJaccardLoss on [B, C, H, W] tensors: the entry points
    of the Function the class must route to, the loss of oracle/losses_oracle.py, the gradient of the reference's chain."""
    K = _K()
    N = K.N
    inp = SC.inputs(case)
    up = SC.upstream(case, inp)
    x, labels, dense, _cw = _tensors(case, inp, dev)
    xs, ls = SC._module_shapes(case, inp)
    target = labels.view(ls) if labels is not None else dense.view(xs)
    crit = _module(case).to(dev)
    with _configured(case) as spy:
        before = N.calls
        loss = crit(x.view(xs), target)
        _backward(dict(loss=loss), up)
        assert N.calls > before
        assert spy.log == SC.entry_points(case), (spy.log, SC.forward_arm(case), SC.backward_arm(case))
    K.flush_label_check()
    want = SC.model(case, inp)
    rv = SC.ratio(loss.detach().cpu().numpy(), want["loss"], **SC.TOL)
    _out64, grad64 = SC.chain_gradient(case, torch.float64, inp, up)
    rg = SC.gradient_ratio(x.grad.cpu().numpy(), grad64, inp["x"])
    _note(case.family, rv, rg)
    print("%s: forward %s, backward %s, value %.3g, gradient %.3g" % (case.name, SC.forward_arm(case), SC.backward_arm(case), rv, rg))
    assert rv <= 1.0 and rg <= 1.0, (rv, rg)


# ------------------------------------------------------------------------------------------------- the kernels that really ran
def _run_module(case, inp, up, dev):
    x, labels, dense, _cw = _tensors(case, inp, dev)
    xs, ls = SC._module_shapes(case, inp)
    loss = _module(case).to(dev)(x.view(xs), labels.view(ls) if labels is not None else dense.view(xs))
    return dict(loss=loss)


def _trace_main():
    """The child process of test_kernels_that_ran_are_the_predicted_ones: every case forward and backward, markers on stderr between the
    runtime's own launch log."""
    dev = torch.device("cuda:0")
    for i, case in enumerate(SC.ALL):
        inp = SC.inputs(case)
        up = SC.upstream(case, inp)
        tensors = _tensors(case, inp, dev)
        with _configured(case):
            torch.cuda.synchronize(dev)
            print("\nSWEEP %d forward" % i, file=sys.stderr, flush=True)
            out = _run_module(case, inp, up, dev) if case.family == "module" else _call(case, *tensors, dev)
            torch.cuda.synchronize(dev)
            print("\nSWEEP %d backward" % i, file=sys.stderr, flush=True)
            if out is not None:
                _backward(out, up)
            torch.cuda.synchronize(dev)
            print("\nSWEEP %d end" % i, file=sys.stderr, flush=True)
    _K().flush_label_check()


def _launched(log_path):
    """{(case index, "forward" | "backward"): [kernel instances of ptb_losses.hip in launch order]} from the child's stderr."""
    ours = {arm.split("<")[0] for c in SC.ALL for arm in (SC.forward_arm(c) + "+" + SC.backward_arm(c)).split("+")} - {"unsupported"}
    ran, key = {}, None
    with open(log_path, errors="replace") as f:
        for line in f:
            m = re.match(r"SWEEP (\d+) (forward|backward|end)", line)
            if m:
                key = None if m.group(2) == "end" else (int(m.group(1)), m.group(2))
                if key is not None:
                    ran[key] = []
                continue
            m = re.search(r"ShaderName : (?:void )?ptb::(\w+)(<[^>]*>)?\(", line)       # (a template instance is printed with its return type)
            if m and key is not None and m.group(1) in ours:
                ran[key].append(m.group(1) + (m.group(2) or "").replace(" ", ""))
    return ran


def test_kernels_that_ran_are_the_predicted_ones(dev, tmp_path):
    log = tmp_path / "launches.log"
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, AMD_LOG_LEVEL="3", PYTHONPATH=os.pathsep.join([os.path.dirname(tests), tests] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    with open(log, "w") as err:
        done = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.DEVNULL, stderr=err, timeout=300)
    assert done.returncode == 0, open(log, errors="replace").read()[-4000:]
    ran = _launched(log)
    assert len(ran) == 2 * len(SC.ALL)
    wrong = []
    for i, case in enumerate(SC.ALL):
        fwd = [a for a in SC.forward_arm(case).split("+") if a != "unsupported"]
        bwd = SC.backward_arm(case).split("+") if fwd else []
        if ran[(i, "forward")] != fwd or ran[(i, "backward")] != bwd:
            wrong.append((case.name, ran[(i, "forward")], fwd, ran[(i, "backward")], bwd))
    assert not wrong, "%d cases launched other kernels than predicted (name, ran, predicted): %s" % (len(wrong), wrong[:5])


if __name__ == "__main__":
    _trace_main()
