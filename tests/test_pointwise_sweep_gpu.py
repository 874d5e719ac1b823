"""GPU half of the sweep of csrc/ptb_pointwise.hip (tests/test_pointwise_sweep_cpu.py is the other half): every case of
tests/pointwise_cases.py through its autograd Function of losses/_pointwise.py -- or through ``_native.launch`` where an output or an
upstream map sits at an element offset -- against the float64 model of oracle/pointwise_oracle.py.

Per case (one family of cases per test; ``pointwise_cases.each`` names every case that fails):
* the sums the Function returns and the slot workspace [64, 4] the forward leaves (which workgroup adds into which slot is part of the
  model), the element-wise / per-pixel / per-row output and, for the public classes, the reduced loss: rtol = atol = 1e-5 (sums and
  slots: atol * max(1, |model|));
* the input gradient for a non-trivial upstream gradient (non-unit scalars on the sums, a random map on the outputs) against the model's
  analytic gradient: rtol 2e-5, atol 1e-5 (bi-tempered: rtol 1e-4, atol 1e-5).  Non-finite model values (QFL at sigmoid(x) == t with
  beta < 1, 0 * log_t(0) at t1 = 1) must be matched in position and kind.  For t2 < 1 the knife edges of the bisection are left out
  (pointwise_cases.KNIFE; at most 1 % of a case, asserted in the CPU file) but must be finite where the model is; nothing else is;
* the native call counter moved by the predicted number of launches and the C entry points called are the predicted ones;
* a second call with other inputs gives that call's own result (nothing is left behind), tunables 1 and 4 go back to 0;
* where a case takes a 16-byte arm, the scalar kernels (tunable 1) agree with it within the same tolerances;
* a launch that writes through an offset view leaves the elements around the view untouched.
One more soft-CE case per forward arm carries a label outside [0, C): the total is NaN, ``flush_label_check()`` raises, the pixel
contributes nothing to the slots, the map and the gradient.  ``ptb_bitempered_rows`` refuses label smoothing at K = 1.  And one child
process runs every case once under the HIP runtime's launch log (AMD_LOG_LEVEL=3): the kernel instances that really ran are the ones
``forward_arm`` / ``backward_arm`` name.

Worst error / tolerance per family (values, gradients), measured on an MI355X with the kernels of commit 08a2645 (this sweep changes none):
    soft_bce 0.062, 0.039   balanced_bce 0.006, 0.013   qfl 0.022, 0.055   wing 0.027, 0.0096   logcosh 0.017, 0.032   soft_f1 0.0043, 0.022
    BalancedElementwise 0.008, 0.0082   SoftCESums 0.026, 0.044   BiTemperedBinarySums 0.056, 0.037   BiTemperedRows 0.075, 0.11
    module 0.0071, 0.027"""
import contextlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pointwise_cases as PC

pytestmark = pytest.mark.gpu

WORST = {}
GUARD = 8                                       # sentinel elements behind every offset view


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nHIP kernels, worst error / tolerance (values, gradients): " + ", ".join("%s %.2g, %.2g" % (k, v[0], v[1]) for k, v in sorted(WORST.items())))


@pytest.fixture(autouse=True)
def _default_tunables():
    """Tunables 1 (scalar kernels) and 4 (loss grid cap) are back at 0 after each test, whatever it did."""
    yield
    lib = _P().N.load()
    for key in PC.TUN_KEYS:
        assert lib.ptb_set_tunable(key, 0) == 0


def _note(family, values, grads):
    old = WORST.get(family, (0.0, 0.0))
    WORST[family] = (max(old[0], values), max(old[1], grads))


def _P():
    from pytorch_toolbelt_amd.losses import _pointwise as P

    return P


class _Spy:
    """The loaded library with a log of the entry points called (every one of them must return 0)."""

    def __init__(self, lib):
        self._lib, self.log = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            rc = fn(*args)
            if name.startswith("ptb_") and name != "ptb_set_tunable":
                self.log.append(name if rc == 0 else "%s:%d" % (name, rc))
            return rc

        return call


@contextlib.contextmanager
def _configured(case):
    """The tunables of a case; the library's entry points under a spy; the slot workspace of every forward kept before it is added up."""
    P = _P()
    N = P.N
    lib = N.load()
    spy = _Spy(lib)
    spy.slots = []
    real_load, real_finalize = N.load, P.finalize

    def finalize(sums, flag=None):
        spy.slots.append(sums.clone())
        return real_finalize(sums, flag)

    try:
        for key, value in zip(PC.TUN_KEYS, case.tun):
            assert lib.ptb_set_tunable(key, value) == 0
        N.load, P.finalize = (lambda: spy), finalize
        yield spy
    finally:
        N.load, P.finalize = real_load, real_finalize
        for key in PC.TUN_KEYS:
            lib.ptb_set_tunable(key, 0)


def _buffer(shape, dtype, off, dev):
    """(allocation, view): a contiguous view of ``shape``, ``off`` elements into an allocation that starts on the 16-byte grid and
    carries GUARD sentinel elements behind the view."""
    n = int(np.prod(shape))
    buf = torch.full((off + n + GUARD,), -777, dtype=dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + n].view(shape)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + off * buf.element_size()
    return buf, view


def _place(a, off, dev):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    _buf, view = _buffer(t.shape, t.dtype, off, dev)
    view.copy_(t)
    return view


def _untouched(buf, off, n):
    return bool((buf[:off] == -777).all()) and bool((buf[off + n:] == -777).all())


def _tensors(case, inp, dev, labels=None):
    o = lambda name: PC.off_of(case, name)                                                   # noqa: E731
    lab = inp["labels"] if labels is None else labels
    return dict(x=_place(inp["x"], o("x"), dev), t=_place(inp["t"], o("t"), dev), labels=_place(lab, o("labels"), dev),
                cw=_place(inp["chan_w"], 0, dev), cpw=_place(inp["chan_pw"], 0, dev), w=_place(inp["w"], 0, dev))


def _up(up, key, dev):
    return torch.from_numpy(np.asarray(up[key])).to(dev)


def _forward(case, T, dev):
    """{key: tensor} of what the Function of a case returns, keys as in ``pointwise_cases.model``."""
    P = _P()
    fam, ign = case.family, case.ignore
    if fam == "PointwiseSums":
        C, HW = PC.kernel_chw(case)
        p0, p1, p2 = PC.kernel_params(case)
        sums, elem = P.PointwiseSums.apply(T["x"], T["t"], T["cw"], T["cpw"], case.kind, case.flags, p0, p1, p2, float(ign or 0.0), C, HW, case.elem)
        return dict(sums=sums, elem=elem) if case.elem else dict(sums=sums)
    if fam == "BalancedElementwise":
        return dict(elem=P.BalancedElementwise.apply(T["x"], T["t"], T["w"], case.flags, float(ign or 0.0)))
    if fam == "SoftCESums":
        total, pix = P.SoftCESums.apply(T["x"], T["labels"], case.eps, ign is not None, int(ign or 0), case.elem)
        return dict(sums=total.reshape(1), elem=pix) if case.elem else dict(sums=total.reshape(1))
    if fam == "BiTemperedBinarySums":
        total, elem = P.BiTemperedBinarySums.apply(T["x"], T["t"], case.t1, case.t2, case.smoothing, 5, ign is not None, float(ign or 0.0), case.elem)
        return dict(sums=total.reshape(1), elem=elem) if case.elem else dict(sums=total.reshape(1))
    assert fam == "BiTemperedRows", fam
    return dict(elem=P.BiTemperedRows.apply(T["x"], T["t"], case.t1, case.t2, case.smoothing, 5))


def _run_function(case, inp, up, dev, labels=None, backward=True):
    """Forward (and backward) of a case through its autograd Function: numpy results, keys as in ``model``."""
    T = _tensors(case, inp, dev, labels)
    T["x"].requires_grad_(backward)
    out = _forward(case, T, dev)
    if backward:
        total = None
        for k, v in out.items():
            g = _up(up, k, dev)
            term = (v * (g[:v.numel()] if k == "sums" else g).to(v.dtype)).sum().double()
            total = term if total is None else total + term
        total.backward()
    got = {k: v.detach().cpu().numpy() for k, v in out.items()}
    if backward:
        got["grad"] = T["x"].grad.cpu().numpy()
    return got


def _run_direct(case, inp, up, dev):
    """The same through ``_native.launch``: outputs and upstream maps where the case's offsets put them, the coefficients as
    ``fold_map_grad`` would hand them over.  Also checks that nothing around an offset view was written."""
    N = _P().N
    T = _tensors(case, inp, dev)
    fam, ign = case.family, case.ignore
    o = lambda name: PC.off_of(case, name)                                                   # noqa: E731
    x = T["x"]
    n = x.numel()
    g = up["sums"]
    sums = torch.empty((PC.SUM_SLOTS, 4), dtype=torch.float64, device=dev)
    gbuf, grad = _buffer(x.shape, torch.float32, o("grad"), dev)
    got, held = {}, [(gbuf, o("grad"), n)]
    if fam in ("PointwiseSums", "BalancedElementwise"):
        C, HW = PC.kernel_chw(case)
        p0, p1, p2 = PC.kernel_params(case)
        tail = (n, C, HW, case.flags, p0, p1, p2, float(ign or 0.0))
        obuf, out = _buffer(x.shape, torch.float32, o("out"), dev)
        held.append((obuf, o("out"), n))
        ge = _place(up["elem"] + (g[0] if fam == "PointwiseSums" else 0), o("grad_elem"), dev)
        if fam == "PointwiseSums":
            N.launch("ptb_pointwise_loss_fwd", dev, case.kind, x.data_ptr(), T["t"].data_ptr(), N.ptr(T["cw"]), N.ptr(T["cpw"]), sums.data_ptr(),
                     out.data_ptr() if case.elem else None, *tail)
            got["slots"] = sums.cpu().numpy()
            got["sums"] = got["slots"].sum(axis=0)
            k = np.array([1.0, g[1]] if case.elem else [g[0], g[1]], dtype=np.float32) * (-1.0 if case.kind == PC.BALANCED_BCE else 1.0)
            coef = torch.from_numpy(k).to(dev)
            N.launch("ptb_pointwise_loss_apply", dev, case.kind, 0, x.data_ptr(), T["t"].data_ptr(), N.ptr(T["cw"]), N.ptr(T["cpw"]), coef.data_ptr(),
                     ge.data_ptr() if case.elem else None, grad.data_ptr(), *tail)
        else:
            N.launch("ptb_pointwise_loss_apply", dev, PC.BALANCED_BCE, 1, x.data_ptr(), T["t"].data_ptr(), None, None, T["w"].data_ptr(), None, out.data_ptr(), *tail)
            N.launch("ptb_pointwise_loss_apply", dev, PC.BALANCED_BCE, 0, x.data_ptr(), T["t"].data_ptr(), None, None, T["w"].data_ptr(), ge.data_ptr(),
                     grad.data_ptr(), *tail)
        if PC.has_map(case):
            got["elem"] = out.cpu().numpy()
    else:
        assert fam == "SoftCESums", fam
        B, C, HW = case.B, case.C, case.HW
        flag = torch.empty(1, dtype=torch.int32, device=dev)
        pbuf, pix = _buffer((B, HW), torch.float32, o("pix_out"), dev)
        held.append((pbuf, o("pix_out"), B * HW))
        tail = (B, C, HW, case.eps, 1 if ign is not None else 0, int(ign or 0))
        N.launch("ptb_soft_ce_fwd", dev, x.data_ptr(), T["labels"].data_ptr(), sums.data_ptr(), pix.data_ptr() if case.elem else None, flag.data_ptr(), *tail)
        got["slots"] = sums.cpu().numpy()
        s = got["slots"].sum(axis=0)
        got["sums"] = np.array([(1.0 - case.eps) * s[0] + case.eps / C * s[1]])
        assert int(flag.item()) == 0
        if case.elem:
            got["elem"] = pix.cpu().numpy()
        gp = _place(up["elem"] + g[0], o("grad_pix"), dev)
        coef = torch.tensor([1.0 if case.elem else float(g[0])], dtype=torch.float32, device=dev)
        N.launch("ptb_soft_ce_bwd", dev, x.data_ptr(), T["labels"].data_ptr(), coef.data_ptr(), gp.data_ptr() if case.elem else None, grad.data_ptr(), *tail)
    got["grad"] = grad.cpu().numpy()
    for buf, off, count in held:
        assert _untouched(buf, off, count), "%s: a launch wrote outside its output" % case.name
    return got


def _run(case, inp, up, dev):
    return _run_direct(case, inp, up, dev) if PC.direct(case) else _run_function(case, inp, up, dev)


def _ratios(case, got, want):
    """(worst value ratio, gradient ratio) of a result against the model, knife edges left out but finite."""
    keep = PC.kept(case, want)
    kg = None if keep is None else PC.expand_kept(case, keep)
    rv = PC.value_ratios(case, got, want, keep)
    assert rv, "nothing was compared"
    if keep is not None and not keep.all() and "slots" in got:
        # with knife edges left out the model's sums do not apply: the kernel's sums against its own per-element values, slot by slot
        own = PC.slot_sums(case, [got["elem"]])
        rv["slots"] = PC.ratio(got["slots"], own, scale_atol=True, **PC.TOL)
        rv["sums"] = PC.ratio(got["sums"], own.sum(axis=0)[:1], scale_atol=True, **PC.TOL)
    rg = PC.ratio(got["grad"], want["grad"], keep=kg, **PC.grad_tol(case))
    if keep is not None and not keep.all():
        out = ~kg.reshape(-1)
        for k in ("elem", "grad"):
            if k in got:
                sel = (~keep if np.size(got[k]) == keep.size else out) & np.isfinite(np.asarray(want[k]).reshape(-1))
                assert np.isfinite(np.asarray(got[k]).reshape(-1)[sel]).all(), "a left-out element of %s is not finite" % k
    return rv, rg


def _vector_arm(case):
    """The case launches a 16-byte arm, forward or backward."""
    arms = (PC.forward_arm(case) + "+" + PC.backward_arm(case)).split("+")
    return any(re.match(r"pw_(fwd|apply)_kernel<\d,true", a) or a.startswith("soft_ce_kernel<4,") for a in arms)


def _flush():
    from pytorch_toolbelt_amd.losses import _kernels as K

    K.flush_label_check()


@pytest.mark.parametrize("group", sorted(PC.GROUPS))
def test_function_against_the_float64_model(group, dev):
    """Every case of one family (one row of the table above); the failure names each case that missed."""
    PC.each(PC.GROUPS[group], lambda case: _against_the_model(case, dev))


def _against_the_model(case, dev):
    P = _P()
    N = P.N
    inp, up = PC.inputs(case), PC.upstream(case)
    want = PC.model(case, inp, up)
    with _configured(case) as spy:
        before = N.calls
        got = _run(case, inp, up, dev)
        assert N.calls - before == PC.launches(case), (N.calls - before, PC.launches(case))
        assert spy.log == PC.entry_points(case), spy.log
        if spy.slots:
            assert len(spy.slots) == 1
            got["slots"] = spy.slots[0].cpu().numpy()
        # nothing is left behind: other inputs give their own result
        oc = PC.other(case)
        oinp = PC.inputs(oc)
        ogot = _run_function(oc, oinp, up, dev, backward=False) if not PC.direct(case) else None
    _flush()
    assert sorted(k for k in got if k != "grad") == sorted(k for k in want if k in ("sums", "slots", "elem")), sorted(got)
    rv, rg = _ratios(case, got, want)
    _note(PC.family_of(case), max(rv.values()), rg)
    print("%s: forward %s, backward %s, values %s, gradient %.3g" % (case.name, PC.forward_arm(case), PC.backward_arm(case),
                                                                    ", ".join("%s %.3g" % kv for kv in sorted(rv.items())), rg))
    assert all(r <= 1.0 for r in rv.values()), rv
    assert rg <= 1.0, rg
    if ogot is not None:
        owant = PC.model(oc, oinp, up)
        orv = PC.value_ratios(oc, ogot, owant, PC.kept(oc, owant))
        assert orv and all(r <= 1.0 for r in orv.values()), ("the call after", orv)
    if _vector_arm(case):                                       # the scalar kernels on the same tensors
        sc = case._replace(tun=(1, case.tun[1]))
        assert not _vector_arm(sc)
        with _configured(sc):
            sgot = _run(sc, inp, up, dev)
        for k in sgot:
            if k == "slots":
                continue
            tol = PC.grad_tol(case) if k == "grad" else PC.TOL
            r = PC.ratio(got[k], sgot[k], scale_atol=k == "sums", **tol)
            assert r <= 1.0, ("vector and scalar arm differ in " + k, r)


def test_label_outside_the_classes_contributes_nothing_and_is_reported(dev):
    cases = PC.bad_label_cases()
    assert len(cases) >= 7
    PC.each(cases, lambda case: _bad_label(case, dev))


def _bad_label(case, dev):
    flush = _flush
    inp, up = PC.inputs(case), PC.upstream(case)
    flush()
    bad = PC.bad_labels(case, inp)
    want = PC.model(case, inp, up, labels=bad)
    assert want["bad"].sum() == 1
    with _configured(case) as spy:
        got = _run_function(case, inp, up, dev, labels=bad)
        assert np.isnan(got.pop("sums")).all()
        with pytest.raises(RuntimeError, match="Class values must be smaller than num_classes"):
            flush()
        got["slots"] = spy.slots[0].cpu().numpy()
        want.pop("sums")
        rv, rg = _ratios(case, got, want)
        assert all(r <= 1.0 for r in rv.values()) and rg <= 1.0, (rv, rg)
        assert (got["grad"][:, :, case.HW // 2][0] == 0).all()
        clean = _run_function(case, inp, up, dev, backward=False)
        assert np.isfinite(clean["sums"]).all()
        flush()


def test_rows_entry_point_refuses_smoothing_of_one_class(dev):
    P = _P()
    act = torch.randn((4, 1), device=dev)
    hot = torch.ones((4, 1), device=dev)
    before = P.N.calls
    with pytest.raises(RuntimeError):
        P.BiTemperedRows.apply(act, hot, 0.8, 1.2, 0.1, 5)
    assert torch.isfinite(P.BiTemperedRows.apply(act, hot, 0.8, 1.2, 0.0, 5)).all() and P.N.calls == before + 2


def _module_call(case, T):
    """The loss of a module case from the public class (tensors shaped as the class takes them)."""
    from pytorch_toolbelt_amd import losses as L
    from pytorch_toolbelt_amd.losses import functional as LF

    cls, kw = case.module
    kw = dict(kw)
    x, t = T["x"], T["t"]
    B, C, HW = case.B, case.C, case.HW
    if cls == "SoftBCEWithLogitsLoss":
        w = None if T["cw"] is None else T["cw"].view(C, 1, 1)
        pw = None if T["cpw"] is None else T["cpw"].view(C, 1, 1)
        return L.SoftBCEWithLogitsLoss(weight=w, pos_weight=pw, **kw)(x.view(B, C, HW, 1), t.view(B, C, HW, 1))
    if cls == "QualityFocalLoss":
        return L.QualityFocalLoss(**kw)(x, t)
    if cls == "balanced_bce":
        return L.balanced_binary_cross_entropy_with_logits(x, t, **kw)
    if cls == "BinarySoftF1Loss":
        return L.BinarySoftF1Loss(**kw)(x, t)
    if cls == "wing_loss":
        return LF.wing_loss(x, t, **kw)
    if cls == "log_cosh_loss":
        return LF.log_cosh_loss(x, t)
    if cls == "SoftCrossEntropyLoss":
        return L.SoftCrossEntropyLoss(**kw)(x, T["labels"])
    if cls == "BinaryBiTemperedLogisticLoss":
        return L.BinaryBiTemperedLogisticLoss(**kw)(x.view(B, 1, C * HW), t.view(B, 1, C * HW))
    assert cls == "BiTemperedLogisticLoss", cls
    return L.BiTemperedLogisticLoss(**kw)(x, t)


def _run_module(case, inp, up, dev):
    T = _tensors(case, inp, dev)
    T["x"].requires_grad_(True)
    loss = _module_call(case, T)
    g = _up(up, "elem", dev).view(loss.shape) if loss.dim() else float(up["loss"])
    (loss * g).sum().backward()
    return loss.detach().cpu().numpy().reshape(-1), T["x"].grad.cpu().numpy()


def test_public_classes_around_the_sums(dev):
    PC.each(PC.MODULES, lambda case: _public_class(case, dev))


def _public_class(case, dev):
    """The scalar algebra around the sums (mean, normalised QFL, class-balance weights, the F1 tail): the loss of the reduced float64
    functions of the oracle, the gradient of float64 autograd through chain + tail."""
    N = _P().N
    inp, up = PC.inputs(case), PC.upstream(case)
    with _configured(case) as spy:
        before = N.calls
        loss, grad = _run_module(case, inp, up, dev)
        assert N.calls - before == PC.launches(case) and spy.log == PC.entry_points(case), (N.calls - before, spy.log)
    want = PC.module_model(case, inp)
    _loss64, grad64 = PC.module_chain_gradient(case, torch.float64, inp, up)
    rv, rg = PC.ratio(loss, want, **PC.TOL), PC.ratio(grad, grad64, **PC.grad_tol(case))
    _note("module", rv, rg)
    print("%s: forward %s, backward %s, value %.3g, gradient %.3g" % (case.name, PC.forward_arm(case), PC.backward_arm(case), rv, rg))
    assert rv <= 1.0 and rg <= 1.0, (rv, rg)


# ------------------------------------------------------------------------------------------------- the kernels that really ran
def _trace_main():
    """The child process of test_kernels_that_ran_are_the_predicted_ones: every case forward and backward, markers on stderr between the
    runtime's own launch log."""
    dev = torch.device("cuda:0")
    for i, case in enumerate(PC.ALL):
        inp, up = PC.inputs(case), PC.upstream(case)
        with _configured(case):
            torch.cuda.synchronize(dev)
            print("\nSWEEP %d begin" % i, file=sys.stderr, flush=True)
            if case.module is not None:
                _run_module(case, inp, up, dev)
            else:
                _run(case, inp, up, dev)
            torch.cuda.synchronize(dev)
            print("\nSWEEP %d end" % i, file=sys.stderr, flush=True)
    _flush()


def _launched(log_path):
    """{case index: [kernel instances of ptb_pointwise.hip in launch order]} from the child's stderr."""
    ours = {arm.split("<")[0] for c in PC.ALL for arm in (PC.forward_arm(c) + "+" + PC.backward_arm(c)).split("+")}
    ran, key = {}, None
    with open(log_path, errors="replace") as f:
        for line in f:
            m = re.match(r"SWEEP (\d+) (begin|end)", line)
            if m:
                key = None if m.group(2) == "end" else int(m.group(1))
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
        done = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.DEVNULL, stderr=err, timeout=240)
    assert done.returncode == 0, open(log, errors="replace").read()[-4000:]
    ran = _launched(log)
    assert len(ran) == len(PC.ALL)
    wrong = []
    for i, case in enumerate(PC.ALL):
        predicted = (PC.forward_arm(case) + "+" + PC.backward_arm(case)).split("+")
        if ran[i] != predicted:
            wrong.append((case.name, ran[i], predicted))
    assert not wrong, "%d cases launched other kernels than predicted (name, ran, predicted): %s" % (len(wrong), wrong[:5])


if __name__ == "__main__":
    _trace_main()
