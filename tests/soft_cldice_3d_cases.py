"""What the dims=3 soft-clDice tests share: the float64 reference -- the definition as a chain of ``max_pool3d`` on the CPU, autograd for its
gradient -- and ``problem``, built like the 2-D one of soft_cldice_cases.py: every volume that is skeletonised holds distinct, separated values."""
import torch
import torch.nn.functional as F

from soft_cldice_cases import B, assert_separated, grad_bound, grid_planes  # noqa: F401

# below any halo, every position at a border; two 8 x 8 x 32 tiles and a ragged rest in every axis; whole tiles
SHAPES = ((3, 5, 7), (11, 13, 37), (8, 16, 64))
ITERATIONS = (1, 3, 8)


def ref_skeleton(x, k):
    """``softskel_k`` of float64 ``[N, C, D, H, W]``"""
    v, skel = x, None
    for _ in range(k + 1):
        nxt = -torch.maximum(torch.maximum(F.max_pool3d(-v, (3, 1, 1), 1, (1, 0, 0)), F.max_pool3d(-v, (1, 3, 1), 1, (0, 1, 0))),
                             F.max_pool3d(-v, (1, 1, 3), 1, (0, 0, 1)))
        delta = F.relu(v - F.max_pool3d(nxt, 3, 1, 1))
        skel = delta if skel is None else skel + F.relu(delta - skel * delta)
        v = nxt
    return skel


def ref_loss(p, g, k, smooth=1.0):
    """the loss of float64 probabilities and targets ``[B, K, D, H, W]``"""
    sp, st = ref_skeleton(p, k), ref_skeleton(g, k)
    tprec = ((sp * g).sum((0, 2, 3, 4)) + smooth) / (sp.sum((0, 2, 3, 4)) + smooth)
    tsens = ((st * p).sum((0, 2, 3, 4)) + smooth) / (st.sum((0, 2, 3, 4)) + smooth)
    return (1.0 - 2.0 * tprec * tsens / (tprec + tsens)).mean()


def grid_volumes(n, D, H, W, lo, hi, gen):
    return grid_planes(n, D * H, W, lo, hi, gen).reshape(n, D, H, W)


def problem(kind, D, H, W, seed=0):
    """``(y_pred, y_true, mode, kwargs, leaf, p, g)`` as in soft_cldice_cases.problem.  ``kind``: binary | multiclass | multilabel | bf16."""
    gen = torch.Generator().manual_seed(seed)
    mask = lambda *s: (torch.rand(s, generator=gen) > 0.5)                                     # noqa: E731
    if kind == "multiclass":
        # softmax over C = 3, classes [0, 1]: x_1 = -x_0, x_2 = x_0 / 2, so p_0 and p_1 are monotone in x_0 (no independent plane keeps them 1e-5 apart
        # at 105 positions: 3.9e-6); logits on [-4, 4] at the smallest shape, on [-1, 1] above it
        edge = 4 if (D, H, W) == SHAPES[0] else 1
        x0 = grid_volumes(B, D, H, W, -edge, edge, gen)
        x2 = 0.5 * x0
        y_pred = torch.stack([x0, -x0, x2], 1).float()
        labels = torch.randint(0, 3, (B, D, H, W), generator=gen)
        leaf = y_pred.double().requires_grad_(True)
        return y_pred, labels, "multiclass", {"classes": [0, 1]}, leaf, torch.softmax(leaf, 1)[:, :2], torch.stack([labels == 0, labels == 1], 1).double()
    if kind == "multilabel":                                                                   # identity: dense probabilities
        y_pred = grid_volumes(B * 2, D, H, W, 0, 1, gen).reshape(B, 2, D, H, W).float()
        y_true = mask(B, 2, D, H, W).float()
        leaf = y_pred.double().requires_grad_(True)
        return y_pred, y_true, "multilabel", {"from_logits": False}, leaf, leaf, y_true.double()
    y_pred = grid_volumes(B, D, H, W, -4, 4, gen).reshape(B, 1, D, H, W).float()
    if kind == "bf16":
        y_pred = y_pred.bfloat16()
    y_true = mask(B, 1, D, H, W).float()
    leaf = y_pred.double().requires_grad_(True)
    return y_pred, y_true, "binary", {}, leaf, torch.sigmoid(leaf), y_true.double()
