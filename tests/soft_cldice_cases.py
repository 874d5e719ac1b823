"""What the soft-clDice tests share: the float64 reference -- the definition of losses/cldice.py written once as a chain of ``max_pool2d`` on the
CPU, autograd for its gradient -- and inputs that cannot flip a selection between float32 and float64: every plane that is skeletonised
holds a seeded random permutation of equally spaced values, so its sorted values differ by more than 1e-5 (asserted)."""
import torch
import torch.nn.functional as F

SHAPES = ((5, 7), (45, 83), (64, 64))       # below any halo, every position at a border; ragged tiles in both axes for tile sides 16 .. 32; whole tiles
CAP = 8
ITERATIONS = (1, 3, CAP)
B = 2


def ref_skeleton(x, k):
    """``softskel_k`` of float64 ``[N, C, H, W]``"""
    v, skel = x, None
    for _ in range(k + 1):
        nxt = -torch.maximum(F.max_pool2d(-v, (3, 1), 1, (1, 0)), F.max_pool2d(-v, (1, 3), 1, (0, 1)))
        delta = F.relu(v - F.max_pool2d(nxt, 3, 1, 1))
        skel = delta if skel is None else skel + F.relu(delta - skel * delta)
        v = nxt
    return skel


def ref_loss(p, g, k, smooth=1.0):
    """the loss of float64 probabilities and targets ``[B, K, H, W]``"""
    sp, st = ref_skeleton(p, k), ref_skeleton(g, k)
    tprec = ((sp * g).sum((0, 2, 3)) + smooth) / (sp.sum((0, 2, 3)) + smooth)
    tsens = ((st * p).sum((0, 2, 3)) + smooth) / (st.sum((0, 2, 3)) + smooth)
    return (1.0 - 2.0 * tprec * tsens / (tprec + tsens)).mean()


def grid_planes(n, H, W, lo, hi, gen):
    """``[n, H, W]`` float64: each plane a random permutation of ``H W`` equally spaced values, the midpoints of ``[lo, hi]`` cut into ``H W`` cells"""
    N = H * W
    return torch.stack([lo + (hi - lo) * (torch.randperm(N, generator=gen).double() + 0.5) / N for _ in range(n)]).reshape(n, H, W)


def assert_separated(planes):
    for plane in planes.reshape(-1, planes.shape[-2] * planes.shape[-1]):
        assert float(plane.double().sort().values.diff().min()) > 1e-5


def grad_bound(ref, dtype):
    """per element: 1e-5 of the largest reference gradient; a bf16 leaf holds its gradient in bf16, rounded once more: half an ulp, 2^-8 of the value"""
    bound = 1e-5 * ref.abs().max()
    return bound + 2.0 ** -8 * (ref.abs() + bound) if dtype == torch.bfloat16 else bound.expand_as(ref)


def problem(kind, H, W, seed=0):
    """``(y_pred, y_true, mode, kwargs, leaf, p, g)``: the call's arguments on the CPU and, in float64, the leaf ``y_pred.double()`` with the probabilities
    (a function of it) and the targets of the selected classes.  ``kind``: binary | multiclass | multilabel | bf16."""
    gen = torch.Generator().manual_seed(seed)
    mask = lambda *s: (torch.rand(s, generator=gen) > 0.5)                                     # noqa: E731
    if kind == "multiclass":
        # softmax over C = 3, classes [0, 1]: x_1 = -x_0.  Up to 64 positions x_2 is an independent grid plane; beyond that no such plane keeps
        # p_0 and p_1 1e-5 apart (their smallest gap falls like 1 / N^2), so x_2 = x_0 / 2 on [-1, 1]: p_0 and p_1 are monotone in x_0
        if H * W <= 64:
            x0, x2 = grid_planes(B, H, W, -4, 4, gen), grid_planes(B, H, W, -4, 4, gen)
        else:
            x0 = grid_planes(B, H, W, -1, 1, gen)
            x2 = 0.5 * x0
        y_pred = torch.stack([x0, -x0, x2], 1).float()
        labels = torch.randint(0, 3, (B, H, W), generator=gen)
        leaf = y_pred.double().requires_grad_(True)
        p = torch.softmax(leaf, 1)[:, :2]
        g = torch.stack([labels == 0, labels == 1], 1).double()
        return y_pred, labels, "multiclass", {"classes": [0, 1]}, leaf, p, g
    if kind == "multilabel":                                                                   # identity: dense probabilities (i + 0.5) / N
        y_pred = grid_planes(B * 2, H, W, 0, 1, gen).reshape(B, 2, H, W).float()
        y_true = mask(B, 2, H, W).float()
        leaf = y_pred.double().requires_grad_(True)
        return y_pred, y_true, "multilabel", {"from_logits": False}, leaf, leaf, y_true.double()
    y_pred = grid_planes(B, H, W, -4, 4, gen).reshape(B, 1, H, W).float()
    if kind == "bf16":
        y_pred = y_pred.bfloat16()
    y_true = mask(B, 1, H, W).float()
    leaf = y_pred.double().requires_grad_(True)
    return y_pred, y_true, "binary", {}, leaf, torch.sigmoid(leaf), y_true.double()
