"""GPU sweep of csrc/ptb_ensemble.hip (Ensembler / ApplySigmoidTo / ApplySoftmaxTo) and csrc/ptb_stack.hip (stack_reduce with more than 8
planes or a caller's eps, forward and backward) against the float64 operator model of oracle/ensembling_oracle.py, over the case tables of
tests/ensemble_cases.py -- tests/test_ensemble_sweep_cpu.py asserts that those tables reach every arm of the host dispatch and that every
case is conditioned for its tolerance.

Tolerances (no element of any comparison is masked out):
  activated and non-linear values against the float64 model      rtol = atol = 1e-5   (TOL of tests/test_ensembling_gpu.py)
  gradients against torch float64 autograd of the same chain     rtol = 2e-4, atol = 2e-5   (the golden gradient tests)
  ``sum`` without an activation                                  the bits of the float32 sum taken in list order
  ``mean`` without an activation                                 that sum / T at rtol = 1e-6, atol = 1e-7 (and the model at 1e-5)
  half / bfloat16 sources                                        the float64 model rounded once to the source type, within one ulp of it
gmean and logodd of saturating logits are checked for properties only (finite, in [0, 1], no NaN where the model has none): no float32
evaluation meets float64 there (tests/ensemble_cases.py: bounded).

Largest error / tolerance seen on an MI355X per family (printed at the end of a run with -s): elementwise 0.019, softmax 0.13, stack
forward 0.025, stack backward 0.018 -- the figures of the reference's own float32 chain on the same cases (the CPU file) are 0.019,
0.13, 0.026 and 0.020: the hardware exp / log / rcp of the kernels cost nothing measurable."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import ensemble_cases as EC
from oracle import ensembling_oracle as NO

pytestmark = pytest.mark.gpu

WORST = {}
ACT_CODES = {None: 0, "sigmoid": 1, "softmax": 2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture()
def native():
    from pytorch_toolbelt_amd import _native as N

    lib = N.load()
    yield N
    lib.ptb_set_tunable(1, 0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nkernels, worst error / tolerance: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


def _note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), r)


def _within(family, got, ref, tol):
    r = EC.ratio(got, ref, **tol)
    print("%s: error / tolerance = %.3g" % (family, r))
    _note(family, r)
    assert r <= 1.0, (family, r)       # (a NaN on one side only makes r NaN and fails here)


class Fixed(nn.Module):
    """A model whose output is a given tensor -- the very tensor, so that its base pointer reaches the kernel."""

    def __init__(self, t):
        super().__init__()
        self.t = t

    def forward(self, x):
        return {"logits": self.t}


def _on_device(x, dev, offset=0, dtype=torch.float32):
    """``x`` on the device, ``offset`` elements into an allocation that is ``offset`` elements longer."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    if offset:
        buf = torch.zeros(t.numel() + offset, dtype=dtype, device=dev)
        buf[offset:] = t.reshape(-1).to(dev)
        d = buf[offset:].view(t.shape)
    else:
        d = t.to(dev)
    assert d.is_contiguous() and (d.data_ptr() % 16 == 0) == ((offset * d.element_size()) % 16 == 0)
    return d


def _wrap(model, act, temperature, dim):
    from pytorch_toolbelt_amd.inference import ensembling as E

    if act == "sigmoid":
        return E.ApplySigmoidTo(model, temperature=temperature)
    if act == "softmax":
        return E.ApplySoftmaxTo(model, dim=dim, temperature=temperature)
    return model


def _ensembler(case, tensors):
    from pytorch_toolbelt_amd.inference.ensembling import Ensembler

    return Ensembler([_wrap(Fixed(t), case.act, case.temperature, case.dim) for t in tensors], reduction=case.reduction)


def _run_ensemble(case, dev, native):
    """(inputs, result) of a case through Ensembler: ONE launch of ptb_ensemble_reduce."""
    xs = EC.inputs(case)
    dtype = getattr(torch, case.dtype)
    tensors = [_on_device(x, dev, case.offset if i == EC.offset_index(case) else 0, dtype) for i, x in enumerate(xs)]
    native.load().ptb_set_tunable(1, case.scalar)
    before = native.calls
    with torch.no_grad():
        out = _ensembler(case, tensors)(None)["logits"]
    assert native.calls == before + 1, "not one fused launch"
    assert out.dtype == dtype and tuple(out.shape) == case.shape
    return xs, out


def _check_values(case, family, got, xs):
    want = EC.model(case, xs)
    if case.props_only:
        assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0 and not np.isnan(want).any()
        return
    if case.act is None and case.reduction in ("sum", "mean"):
        seq = EC.list_order_sum(xs)
        if case.reduction == "sum":
            assert np.array_equal(got, seq)
        else:
            assert EC.ratio(got, seq / np.float32(case.T), **EC.MEAN_TOL) <= 1.0
    _within(family, got, want, EC.TOL)


# ------------------------------------------------------------------------------------------------- the two ensemble families
@pytest.mark.parametrize("case", EC.ELEMENTWISE, ids=EC.ids)
def test_elementwise_ensemble(case, dev, native):
    """ensemble_kernel<OPK, ACT> and ensemble_scalar_kernel<ACT> (by size, by the alignment of one input, by the tunable)."""
    xs, out = _run_ensemble(case, dev, native)
    _check_values(case, "elementwise", out.cpu().numpy(), xs)


@pytest.mark.parametrize("case", EC.SOFTMAX, ids=EC.ids)
def test_softmax_ensemble(case, dev, native):
    """ensemble_softmax_kernel<OPK, 4 | 8 | 16> on both sides of every bucket bound and the generic kernel (C = 17, HW = 35, an offset
    input, the tunable), over dim 0 / 1 / 2 / -1 of 3-D and 4-D shapes."""
    xs, out = _run_ensemble(case, dev, native)
    _check_values(case, "softmax", out.cpu().numpy(), xs)


@pytest.mark.parametrize("case", EC.LOW_PRECISION, ids=EC.ids)
def test_low_precision_sources(case, dev, native):
    """half / bfloat16 model outputs: the result has the source dtype and is the float64 model of the widened inputs rounded once to
    it, within one ulp of that dtype (the rule of tests/test_volume_tta_gpu.py)."""
    xs, out = _run_ensemble(case, dev, native)
    want = torch.from_numpy(EC.model(case, xs)).to(out.dtype)

    def ordinal(t):      # position of a 16-bit float on the number line of its type (-0 and +0 share one)
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)

    assert not torch.isnan(out).any()
    assert int((ordinal(out.cpu()) - ordinal(want)).abs().max()) <= 1


# ------------------------------------------------------------------------------------------------- stack reduce, forward and backward
def _views():
    from pytorch_toolbelt_amd.inference import _views as V

    return V


@pytest.mark.parametrize("case", EC.STACK, ids=EC.ids)
def test_stack_reduce_and_backward(case, dev, native):
    """stack_reduce_kernel<vector | scalar> and stack_reduce_bwd_kernel<vector | scalar>: 0..4 trips of the four-plane loop with
    remainders 0..3, every reduction, the caller's eps."""
    V = _views()
    xs = EC.inputs(case)
    x = _on_device(xs, dev, case.offset).requires_grad_(True)
    up = EC.grad_weights(case.shape)
    native.load().ptb_set_tunable(1, case.scalar)
    before = native.calls
    out = V.stack_reduce(x, V.REDUCTION_CODES[case.reduction], case.eps)
    assert native.calls == before + 1 and tuple(out.shape) == case.shape
    (out * torch.from_numpy(up).to(dev)).sum().backward()
    assert native.calls == before + 2
    _check_values(case, "stack forward", out.detach().cpu().numpy(), xs)
    want, grad = NO.stack_gradient64(xs, case.reduction, case.eps, up)
    _within("stack forward", out.detach().cpu().numpy(), want, EC.TOL)
    _within("stack backward", x.grad.cpu().numpy(), grad, EC.GRAD_TOL)


# ------------------------------------------------------------------------------------------------- direct C ABI calls
GUARD = -12345.0


def _guarded(n, dev, offset):
    """(buffer of n + offset floats filled with GUARD, pointer ``offset`` elements into it)."""
    buf = torch.full((n + offset,), GUARD, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * offset


@pytest.mark.parametrize("case", [c for c in EC.ELEMENTWISE + EC.SOFTMAX
                                  if c.shape in (EC.ONE_GROUP, (2, 5, 6, 6)) and not (c.offset or c.scalar or c.props_only)], ids=EC.ids)
def test_c_abi_ensemble_output_offset_by_one_element(case, dev, native):
    """ptb_ensemble_reduce with ``out`` one element into a buffer allocated one element longer: the wrappers always hand a fresh
    (aligned) output over, so only the C ABI reaches this side of aligned16."""
    xs = EC.inputs(case)
    ins = [_on_device(x, dev) for x in xs]
    n = EC.numel(case.shape)
    B, C, HW = EC.as_bchw(case.shape, case.act, case.dim)
    buf, out_ptr = _guarded(n, dev, 1)
    ptrs = (ctypes.c_void_p * len(ins))(*[t.data_ptr() for t in ins])
    with native.on_device(dev):
        rc = native.load().ptb_ensemble_reduce(ptrs, len(ins), _views().REDUCTION_CODES[case.reduction], ACT_CODES[case.act], case.temperature,
                                               B, C, HW, out_ptr, native.stream_ptr(dev))
    assert rc == 0
    got = buf.cpu().numpy()
    assert got[0] == GUARD
    _check_values(case, "elementwise" if case.act != "softmax" else "softmax", got[1:].reshape(case.shape), xs)


@pytest.mark.parametrize("which", ["out", "grad_out", "grad", "fwd_out"])
@pytest.mark.parametrize("reduction,T,eps", [("gmean", 9, 1e-6), ("logodd", 5, 0.05), ("sum", 10, 1e-6)])
def test_c_abi_stack_pointers_offset_by_one_element(reduction, T, eps, which, dev, native):
    """ptb_stack_reduce with ``out``, and ptb_stack_reduce_bwd with each of ``out`` / ``grad_out`` / ``grad``, one element into a buffer
    allocated one element longer (stack_reduce allocates all of them itself, always aligned)."""
    case = EC.make_case("stack", EC.ONE_GROUP, T, reduction, eps=eps, seed=400 + T)
    lib, code = native.load(), _views().REDUCTION_CODES[reduction]
    xs = EC.inputs(case)
    n = EC.numel(case.shape)
    src = _on_device(xs.reshape(T, n), dev)
    up = EC.grad_weights((n,))
    want, grad64 = NO.stack_gradient64(xs.reshape(T, n), reduction, eps, up)
    off = {k: int(which == k) for k in ("out", "grad_out", "grad", "fwd_out")}
    out_buf, out_ptr = _guarded(n, dev, off["out"] or off["fwd_out"])
    with native.on_device(dev):
        assert lib.ptb_stack_reduce(src.data_ptr(), T, n, code, eps, out_ptr, native.stream_ptr(dev)) == 0
    got = out_buf.cpu().numpy()
    _within("stack forward", got[len(got) - n:], want, EC.TOL)
    if which == "fwd_out":
        assert got[0] == GUARD
        return
    g_buf, g_ptr = _guarded(n, dev, off["grad_out"])
    g_buf[off["grad_out"]:] = torch.from_numpy(up).to(dev)
    grad_buf, grad_ptr = _guarded(T * n, dev, off["grad"])
    with native.on_device(dev):
        assert lib.ptb_stack_reduce_bwd(src.data_ptr(), out_ptr, g_ptr, T, n, code, eps, grad_ptr, native.stream_ptr(dev)) == 0
    got = grad_buf.cpu().numpy()
    if off["grad"]:
        assert got[0] == GUARD
    if off["grad_out"]:
        assert float(g_buf[0]) == GUARD
    _within("stack backward", got[len(got) - T * n:].reshape(T, n), grad64, EC.GRAD_TOL)


# ------------------------------------------------------------------------------------------------- second trips of the capped grids
def _device_ratio(got, ref, rtol, atol):
    return float(((got.double() - ref).abs() / (atol + rtol * ref.abs())).max())


def test_stack_second_grid_trip(dev, native):
    """n / 4 = 256 * 16 * 256 + 300 lanes: the last 300 lanes of stack_reduce_kernel<vector> and of its backward are produced by the second
    trip of the grid-stride loop.  Reference: torch float64 on the device; the last 1200 elements are compared on their own."""
    case = EC.SECOND_TRIP_STACK
    V = _views()
    n, T = case.shape[0], case.T
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.rand((T, n), device=dev, generator=g) * 0.98 + 0.01
    probes = torch.tensor(EC.CLAMP_PROBES + EC.EPS_PROBES, device=dev)
    x[0, :8], x[T - 1, n - 8:] = probes, probes
    x.requires_grad_(True)
    up = (torch.arange(n, device=dev) % 5 + 1).float()
    before = native.calls
    out = V.stack_reduce(x, V.REDUCTION_CODES[case.reduction], case.eps)
    (out * up).sum().backward()
    assert native.calls == before + 2
    x64 = x.detach().double().requires_grad_(True)
    ref = NO.torch_chain(x64, case.reduction, case.eps)
    (ref * up.double()).sum().backward()
    ref = ref.detach()
    for name, sl in (("tail", slice(n - EC.TAIL, n)), ("all", slice(0, n))):
        r = _device_ratio(out.detach()[sl], ref[sl], **EC.TOL)
        rg = _device_ratio(x.grad[:, sl], x64.grad[:, sl], **EC.GRAD_TOL)
        print("second trip (%s): forward %.3g, backward %.3g of the tolerance" % (name, r, rg))
        _note("stack forward", r)
        _note("stack backward", rg)
        assert r <= 1.0 and rg <= 1.0, (name, r, rg)


def test_softmax_ensemble_second_grid_trip(dev, native):
    """B * HW / 4 = 16384 * 256 + 300 lanes of ensemble_softmax_kernel<0, 4, 4>: the last 300 pixel groups of the last batch element are
    produced by the second trip.  Reference: torch float64 on the device, one batch element at a time; the last 1200 pixels of every class
    plane of the last batch element (which hold the last 1200 elements) are compared on their own."""
    case = EC.SECOND_TRIP_SOFTMAX
    g = torch.Generator(device=dev).manual_seed(8)
    xs = [torch.randn(case.shape, device=dev, generator=g) * 3 for _ in range(case.T)]
    before = native.calls
    with torch.no_grad():
        out = _ensembler(case, xs)(None)["logits"]
    assert native.calls == before + 1
    B, HW = case.shape[0], case.shape[2]
    for b in range(B):
        ref = sum(x[b].mul(case.temperature).double().softmax(dim=0) for x in xs) / case.T
        if b == B - 1:
            r = _device_ratio(out[b][:, HW - EC.TAIL:], ref[:, HW - EC.TAIL:], **EC.TOL)
            print("second trip (tail): %.3g of the tolerance" % r)
            assert r <= 1.0, r
            assert _device_ratio(out.view(-1)[-EC.TAIL:], ref.reshape(-1)[-EC.TAIL:], **EC.TOL) <= 1.0
        r = _device_ratio(out[b], ref, **EC.TOL)
        _note("softmax", r)
        assert r <= 1.0, (b, r)
        del ref


# ------------------------------------------------------------------------------------------------- routing of Ensembler
@pytest.mark.parametrize("act,reduction", [(None, "mean"), ("sigmoid", "gmean"), ("softmax", "hmean")])
def test_sixteen_models_are_one_launch_seventeen_take_the_stack_path(act, reduction, dev, native):
    for T in (16, 17):
        case = EC.make_case("softmax" if act == "softmax" else "elementwise", (2, 5, 6, 6), T, reduction, act=act, temperature=0.5, seed=500 + T)
        xs = EC.inputs(case)
        tensors = [_on_device(x, dev) for x in xs]
        before = native.calls
        with torch.no_grad():
            out = _ensembler(case, tensors)(None)["logits"]
        launches = native.calls - before
        if T == 16:
            assert launches == 1
        else:       # one activation launch per wrapped model, then ptb_stack_reduce over the stack
            assert launches == (T if act else 0) + 1
        _within("elementwise" if T == 16 and act != "softmax" else ("softmax" if T == 16 else "stack forward"), out.cpu().numpy(),
                EC.model(case, xs), EC.TOL)


@pytest.mark.parametrize("reduction", ["mean", "log1p", "hmean"])
def test_models_with_different_wrappers_in_one_ensemble(reduction, dev, native):
    """sigmoid-, softmax- and un-wrapped models in one list: each activation is applied on its own, then one list reduce."""
    from pytorch_toolbelt_amd.inference.ensembling import Ensembler

    shape = (2, 5, 6, 6)
    wraps = [("sigmoid", 2.0, 1), ("softmax", 0.5, 1), (None, 1.0, 1), ("softmax", 1.0, -1), ("sigmoid", 1.0, 1)]
    xs = [EC.inputs(EC.make_case("softmax" if a == "softmax" else "elementwise", shape, 1, "mean", act=a, temperature=t, dim=d, seed=600 + i))[0]
          for i, (a, t, d) in enumerate(wraps)]
    models = [_wrap(Fixed(_on_device(x, dev)), a, t, d) for x, (a, t, d) in zip(xs, wraps)]
    before = native.calls
    with torch.no_grad():
        out = Ensembler(models, reduction=reduction)(None)["logits"]
    assert native.calls == before + 4 + 1
    want = NO.ensemble64(xs, reduction, [w[0] for w in wraps], [w[1] for w in wraps], [w[2] for w in wraps])
    _within("elementwise", out.cpu().numpy(), want, EC.TOL)


@pytest.mark.parametrize("reduction", EC.NONLINEAR)
def test_inputs_that_require_grad_take_the_differentiable_path(reduction, dev, native):
    """T = 9 model outputs that require grad: torch.stack + the differentiable stack reduce; values equal the model, gradients equal
    float64 autograd of the reference's chain."""
    from pytorch_toolbelt_amd.inference.ensembling import Ensembler

    case = EC.make_case("stack", EC.ONE_GROUP, 9, reduction, seed=700)
    xs = EC.inputs(case)
    leaves = [_on_device(x, dev).requires_grad_(True) for x in xs]
    up = EC.grad_weights(case.shape)
    out = Ensembler([Fixed(t) for t in leaves], reduction=reduction)(None)["logits"]
    assert out.requires_grad
    (out * torch.from_numpy(up).to(dev)).sum().backward()
    want, grad = NO.stack_gradient64(xs, reduction, case.eps, up)
    _within("stack forward", out.detach().cpu().numpy(), want, EC.TOL)
    _within("stack backward", np.stack([t.grad.cpu().numpy() for t in leaves]), grad, EC.GRAD_TOL)
