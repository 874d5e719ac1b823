"""CPU: utils/_maps.py is the one host layer of the label-map tools -- no tool module takes an underscore name from a sibling other than it --,
its lower-envelope pass gives the same minima with and without the feature index, and its rule for writing ``out=`` directly holds."""
import ast
from pathlib import Path

import numpy as np
import pytest
import torch

from pytorch_toolbelt_amd.utils import _maps as M

PKG = Path(M.__file__).resolve().parents[1]
MODULES = sorted((PKG / "utils").glob("*.py")) + [PKG / "losses" / "distance_losses.py"]
SIBLINGS = {p.stem for p in (PKG / "utils").glob("*.py")} - {"__init__", "_maps"}


def _private(name):
    return name.startswith("_") and not (name.startswith("__") and name.endswith("__"))


@pytest.mark.parametrize("path", MODULES, ids=lambda p: p.stem)
def test_no_underscore_name_comes_from_a_sibling_but_maps(path):
    tree = ast.parse(path.read_text())
    aliases = {}
    for node in ast.walk(tree):
        if not isinstance(node, ast.ImportFrom) or node.level == 0:
            continue
        source = (node.module or "").split(".")[-1]
        if source in SIBLINGS:                                    # from .components import ...
            taken = [a.name for a in node.names if _private(a.name)]
            assert not taken, f"{path.name} imports {taken} from {source}: shared helpers live in _maps"
        elif source in ("", "utils"):                             # from . import distance as _distance
            aliases.update({a.asname or a.name: a.name for a in node.names if a.name in SIBLINGS})
    reads = [f"{node.value.id}.{node.attr}" for node in ast.walk(tree)
             if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in aliases and _private(node.attr)]
    assert not reads, f"{path.name} reads {reads} through a sibling module: shared helpers live in _maps"
    assert MODULES and "components" in SIBLINGS and "_maps" not in SIBLINGS


def _brute(f, weight, inf):
    n = f.shape[1]
    i = np.arange(n)
    cost = f[:, None, :] + weight * (i[:, None] - i[None, :]) ** 2                # [line, i, j]
    g = np.minimum(cost.min(axis=2), inf)
    return g, np.where(g >= inf, -1, cost.argmin(axis=2))                     # (argmin: the first, so the smallest, minimising j)


LINES = {"no site": [0, 0, 0, 0, 0, 0, 0], "all sites": [1, 1, 1, 1, 1, 1, 1], "one site": [0, 0, 0, 0, 0, 1, 0], "ends": [1, 0, 0, 0, 0, 0, 1],
         "ties on both sides": [1, 0, 0, 0, 1, 0, 0], "even gaps": [0, 1, 0, 0, 1, 0, 1], "first only": [1, 0, 0, 0, 0, 0, 0]}


@pytest.mark.parametrize("kind", ["int64", "float64", "float64 weight 2.25"])
def test_envelope_host_gives_the_same_minima_with_and_without_the_feature(kind):
    sites = np.array(list(LINES.values()), bool)
    if kind == "int64":
        inf, weight = M.HOST_INF, 1
        f = np.where(sites, 0, inf).astype(np.int64)
    else:
        inf, weight = np.inf, 2.25 if kind.endswith("2.25") else 1.0
        f = np.where(sites, 0.0, inf)
    f[2, 5] = 3                                                   # a second pass sees values other than 0 and inf
    feat = np.where(f != inf, np.arange(f.shape[1], dtype=np.int64)[None, :], -1)
    want_g, want_h = _brute(f, weight, inf)
    g, none = M.envelope_host(f, weight, inf)
    g2, h = M.envelope_host(f, weight, inf, feat)
    assert none is None and g.dtype == f.dtype and g2.dtype == f.dtype
    assert np.array_equal(g, g2), kind
    assert np.array_equal(g, want_g), kind
    assert np.array_equal(np.where(g2 >= inf, -1, h), want_h), kind
    assert np.array_equal(g[0], f[0]) and not g[1].any()          # no site: untouched; all sites: all zero
    assert h[4, 2] == 0 and h[4, 5] == 4 and h[4, 6] == 4         # a tie takes the smaller index, whichever side it lies on
    empty = f[:1]
    assert M.envelope_host(empty, weight, inf)[0] is empty


def test_direct_out_rule():
    x = torch.zeros((8, 16), dtype=torch.int32)
    out = torch.zeros((8, 16), dtype=torch.int32)
    assert out.data_ptr() % 16 == 0
    assert M.direct_out(out) and M.direct_out(out, x) and M.direct_out(out, x, None)
    assert not M.direct_out(None) and not M.direct_out(None, x)
    assert not M.direct_out(out.t()) and not M.direct_out(out[:, ::2])                         # not contiguous
    shifted = torch.zeros(8 * 16 + 4, dtype=torch.int32)[1:1 + 8 * 16].reshape(8, 16)           # contiguous, 4 bytes off
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4 and not M.direct_out(shifted)
    assert not M.direct_out(x, x) and not M.direct_out(out, None, out)
    block = torch.zeros((2, 8, 16), dtype=torch.int32)                                          # two aligned halves of one storage
    assert M.direct_out(block[1]) and not M.direct_out(block[1], block[0]) and M.direct_out(block[1], x)
    same = torch.zeros((8, 16), dtype=torch.int32)
    assert M.finish_out(None, x) is x and M.finish_out(x, x) is x
    x[0, 0] = 7
    assert M.finish_out(same, x) is same and same[0, 0] == 7
