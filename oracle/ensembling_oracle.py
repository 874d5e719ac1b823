"""Oracle (test infrastructure only) for inference/ensembling.py of the reference: numpy restatement.

Citations are ``pytorch_toolbelt/inference/ensembling.py:LINE``."""
import numpy as np

from . import tta_oracle as AO


def sigmoid_to(x, temperature=1.0):
    """ApplySigmoidTo.forward, :62-66: ``output.mul(temperature).sigmoid_()`` in float32."""
    z = (np.asarray(x, dtype=np.float32) * np.float32(temperature)).astype(np.float64)
    return (1.0 / (1.0 + np.exp(-z))).astype(np.float32)


def softmax_to(x, temperature=1.0, dim=1):
    """ApplySoftmaxTo.forward, :38-42: ``output.mul(temperature).softmax(dim)``; float64 internally, float32 out."""
    z = (np.asarray(x, dtype=np.float32) * np.float32(temperature)).astype(np.float64)
    z = z - z.max(axis=dim, keepdims=True)
    e = np.exp(z)
    return (e / e.sum(axis=dim, keepdims=True)).astype(np.float32)


def ensemble(outputs, reduction="mean"):
    """Ensembler.forward for one key, :108-117: ``torch.stack(outputs)`` then ``_deaugment_averaging`` over dim 0."""
    return AO.deaugment_averaging(np.stack([np.asarray(o, dtype=np.float32) for o in outputs]), reduction)


# ------------------------------------------------------------------------------------------------- float64 operator model
# Every operation of the family is post(mean_t(pre(act(x_t * temperature)))) -- ``fn.py`` = pytorch_toolbelt/inference/functional.py,
# ``tta.py`` = pytorch_toolbelt/inference/tta.py:63-95.  The model takes the float32 inputs, forms the product with the temperature in
# float32 (what ``output.mul(temperature)`` yields) and evaluates everything after it in float64.
REDUCTIONS = ("sum", "mean", "gmean", "hmean", "harmonic1p", "logodd", "log1p")
DEFAULT_EPS = 1e-6


def clamp_bounds(eps=DEFAULT_EPS):
    """(lo, hi) of ``clamp(min=eps, max=1.0 - eps)`` on a float32 tensor: torch rounds the Python doubles to float32, so the bounds
    are float32(eps) and float32(1.0 - eps) -- 0.99999899 for the default eps, not 1 - 1e-6 (which moves logodd at the clamp by 1 %)."""
    return float(np.float32(eps)), float(np.float32(1.0 - eps))


def activate64(x, act=None, temperature=1.0, dim=1):
    """float64 value of the wrapper's activation on the float32 tensor ``x``: None, "sigmoid" (:62-66) or "softmax" over ``dim`` (:38-42)."""
    x = np.asarray(x, dtype=np.float32)
    if act is None:
        return x.astype(np.float64)
    z = (x * np.float32(temperature)).astype(np.float64)
    if act == "sigmoid":
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-z))
    if act == "softmax":
        e = np.exp(z - z.max(axis=dim, keepdims=True))
        return e / e.sum(axis=dim, keepdims=True)
    raise KeyError(act)


def reduce64(p, reduction, eps=DEFAULT_EPS):
    """The reduction over axis 0 of the float64 stack ``p [T, ...]``: tta.py:63-95 with the formulas of fn.py:250-333."""
    p = np.asarray(p, dtype=np.float64)
    lo, hi = clamp_bounds(eps)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if reduction == "sum":
            return p.sum(axis=0)
        if reduction == "mean":
            return p.mean(axis=0)
        if reduction in ("gmean", "geometric_mean"):
            return np.exp(np.log(p).mean(axis=0))                                     # fn.py:261
        if reduction in ("hmean", "harmonic_mean"):
            return 1.0 / np.maximum((1.0 / np.maximum(p, lo)).mean(axis=0), lo)       # fn.py:275-277
        if reduction == "harmonic1p":
            return 1.0 / (1.0 / (p + 1.0)).mean(axis=0) - 1.0                         # fn.py:292-294
        if reduction == "logodd":
            q = np.clip(p, lo, hi)                                                    # fn.py:311-314
            e = np.exp(np.log(q / (1.0 - q)).mean(axis=0))
            return e / (1.0 + e)
        if reduction == "log1p":
            return np.exp(np.log1p(p).mean(axis=0)) - 1.0                             # fn.py:330-332
    raise KeyError(reduction)


def ensemble64(outputs, reduction="mean", act=None, temperature=1.0, dim=1, eps=DEFAULT_EPS):
    """float64 model of reduce_t act(outputs[t] * temperature); ``act`` / ``temperature`` / ``dim`` may be one value for every model
    or a list with one entry per model (an ensemble of differently wrapped models)."""
    T = len(outputs)

    def per_model(v):
        return list(v) if isinstance(v, (list, tuple)) else [v] * T

    acts, temps, dims = per_model(act), per_model(temperature), per_model(dim)
    return reduce64(np.stack([activate64(o, a, t, d) for o, a, t, d in zip(outputs, acts, temps, dims)]), reduction, eps)


def torch_chain(stack, reduction, eps=DEFAULT_EPS):
    """The reference's own op chain on a torch stack ``[T, ...]`` of any float dtype (tta.py:63-95, fn.py:250-333, op for op): the
    float32 evaluation whose distance from the float64 model says how well a case is conditioned, and -- on a float64 stack that
    requires grad -- the autograd reference of the gradients.  A float64 stack is clamped at the float32 bounds of clamp_bounds()."""
    import torch

    x = stack
    lo, hi = clamp_bounds(eps) if x.dtype == torch.float64 else (eps, 1.0 - eps)
    if reduction == "sum":
        return x.sum(dim=0)
    if reduction == "mean":
        return x.mean(dim=0)
    if reduction in ("gmean", "geometric_mean"):
        return x.log().mean(dim=0).exp()
    if reduction in ("hmean", "harmonic_mean"):
        return torch.reciprocal(torch.mean(torch.reciprocal(x.clamp_min(lo)), dim=0).clamp_min(lo))
    if reduction == "harmonic1p":
        return torch.reciprocal(torch.mean(torch.reciprocal(x + 1), dim=0)) - 1
    if reduction == "logodd":
        x = x.clamp(min=lo, max=hi)
        x = torch.mean(torch.log(x / (1 - x)), dim=0)
        return torch.exp(x) / (1 + torch.exp(x))
    if reduction == "log1p":
        return torch.exp(torch.mean(torch.log1p(x), dim=0)) - 1
    raise KeyError(reduction)


def torch_activate(x, act=None, temperature=1.0, dim=1):
    """ApplySigmoidTo / ApplySoftmaxTo on a torch tensor, op for op (:38-42, :62-66)."""
    if act is None:
        return x
    return x.mul(temperature).sigmoid_() if act == "sigmoid" else x.mul(temperature).softmax(dim=dim)


def stack_gradient64(stack, reduction, eps, upstream):
    """d sum(out * upstream) / d stack by torch float64 autograd of torch_chain on the CPU; ``stack`` float32 numpy [T, ...]."""
    import torch

    x = torch.from_numpy(np.asarray(stack, dtype=np.float32)).double().requires_grad_(True)
    out = torch_chain(x, reduction, eps)
    (out * torch.from_numpy(np.asarray(upstream, dtype=np.float64)).reshape(out.shape)).sum().backward()
    return out.detach().numpy(), x.grad.numpy()
