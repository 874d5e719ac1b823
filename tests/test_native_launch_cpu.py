"""CPU: ``_native.launch`` is the one way the package calls a stream-taking entry point of libptb_hip.so -- no other module makes a device
current, fetches a stream or counts a call on its own, but for the exceptions listed here --, and it keeps its protocol: the stream last,
the device it was given, one counted call, the code checked or handed back."""
import ast
import contextlib
from collections import Counter
from pathlib import Path

import pytest
import torch

from pytorch_toolbelt_amd import _native as N

PKG = Path(N.__file__).resolve().parent
MODULES = sorted(p for p in PKG.rglob("*.py") if p != PKG / "_native.py")
PROTOCOL = ("stream_ptr", "bump", "on_device")

# (module, function, what it does) -> why it does not go through launch; every entry must still occur, exactly once
EXCEPTIONS = {
    ("inference/_merge_modes.py", "take_slim", "calls +="): "the ~4 us call per batch of a deferred image: a cached function pointer, hand-tuned",
    ("parallel.py", "__init__", "on_device"): "brackets ptb_rccl_comm_init, which takes no stream",
    ("parallel.py", "post", "on_device"): "ptb_halo_exchange runs on the exchange's own stream, not on the current one",
    ("parallel.py", "post", "bump"): "the same call: counted by hand",
}


class _Walk(ast.NodeVisitor):
    def __init__(self, tree):
        self.aliases, self.names, self.found, self.stack = set(), {}, [], []
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom):
                if (node.module or "").split(".")[-1] == "_native":           # from .._native import bump
                    self.names.update({a.asname or a.name: a.name for a in node.names})
                else:                                                         # from .. import _native as N
                    self.aliases.update(a.asname or a.name for a in node.names if a.name == "_native")
            elif isinstance(node, ast.Import):
                self.aliases.update(a.asname for a in node.names if a.name.endswith("._native") and a.asname)
        self.visit(tree)

    def _native_attr(self, node):
        """the name ``node`` reads from _native, through an alias of the module or a name imported from it"""
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in self.aliases:
            return node.attr
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Attribute) and node.value.attr == "_native":
            return node.attr                                                  # pytorch_toolbelt_amd._native.bump
        if isinstance(node, ast.Name):
            return self.names.get(node.id)
        return None

    def _note(self, what):
        self.found.append((self.stack[-1] if self.stack else "<module>", what))

    def visit_FunctionDef(self, node):
        self.stack.append(node.name)
        self.generic_visit(node)
        self.stack.pop()

    visit_AsyncFunctionDef = visit_FunctionDef

    def visit_Call(self, node):
        if self._native_attr(node.func) in PROTOCOL:
            self._note(self._native_attr(node.func))
        self.generic_visit(node)

    def _store(self, target):
        if self._native_attr(target) == "calls":
            self._note("calls +=")

    def visit_Assign(self, node):
        for t in node.targets:
            self._store(t)
        self.generic_visit(node)

    def visit_AugAssign(self, node):
        self._store(node.target)
        self.generic_visit(node)

    def visit_Attribute(self, node):
        if node.attr == "_cuda_getCurrentRawStream":
            self._note("raw stream lookup")
        self.generic_visit(node)

    def visit_Constant(self, node):
        if node.value == "_cuda_getCurrentRawStream":                         # getattr(torch._C, "...", None)
            self._note("raw stream lookup")


def _findings(source):
    return _Walk(ast.parse(source)).found


def test_the_walk_sees_every_form():
    src = ("from .. import _native as N\nfrom .._native import bump as b, calls\nimport torch\n"
           "def f(d):\n    with N.on_device(d):\n        s = N.stream_ptr(d)\n    b()\n    N.calls += 1\n    N.calls = 0\n"
           "    r = getattr(torch._C, '_cuda_getCurrentRawStream', None)\n    return torch._C._cuda_getCurrentRawStream\n"
           "def g():\n    N.launch('ptb_x', None)\n    return N.calls, N.check, N.load\n")
    assert Counter(_findings(src)) == Counter({("f", "on_device"): 1, ("f", "stream_ptr"): 1, ("f", "bump"): 1, ("f", "calls +="): 2,
                                               ("f", "raw stream lookup"): 2})


def test_only_launch_speaks_the_launch_protocol():
    found = Counter()
    for path in MODULES:
        rel = path.relative_to(PKG).as_posix()
        found.update((rel, fn, what) for fn, what in _findings(path.read_text()))
    assert len(MODULES) > 40 and (PKG / "losses" / "_kernels.py") in MODULES
    stray = {k: n for k, n in found.items() if k not in EXCEPTIONS}
    assert not stray, f"call the entry point through _native.launch (or list the exception with its reason): {stray}"
    gone = [k for k in EXCEPTIONS if found[k] != 1]
    assert not gone, f"listed exceptions that no longer occur exactly once: {gone}"


class _Lib:
    def __init__(self, code):
        self.code, self.seen = code, []

    def ptb_fake(self, *args):
        self.seen.append(args)
        return self.code

    def ptb_last_hip_error(self):
        return b""


@pytest.fixture
def stub(monkeypatch):
    """``launch`` over a recording library: ``(run, log)`` -- ``run(code, *args, **kw)`` returns (result or raised exception, calls added, lib)"""
    log = []
    sentinel, device = object(), torch.device("cpu")

    @contextlib.contextmanager
    def on_device(dev):
        log.append(("on_device", dev))
        yield

    def stream_ptr(dev):
        log.append(("stream_ptr", dev))
        return sentinel

    monkeypatch.setattr(N, "on_device", on_device)
    monkeypatch.setattr(N, "stream_ptr", stream_ptr)

    def run(code, *args, **kw):
        lib = _Lib(code)
        monkeypatch.setattr(N, "_lib", lib)
        before = N.calls
        try:
            res = N.launch("ptb_fake", device, *args, **kw)
        except Exception as e:                                                # noqa: BLE001 (the test looks at what was raised)
            res = e
        return res, N.calls - before, lib

    run.sentinel, run.device = sentinel, device
    return run, log


def test_launch_passes_the_arguments_then_the_stream_of_its_device(stub):
    run, log = stub
    a, b = object(), [1, 2]
    res, added, lib = run(0, a, 7, None, b, 2.5)
    assert res is None and added == 1
    (seen,) = lib.seen
    assert len(seen) == 6 and seen[-1] is run.sentinel
    assert seen[0] is a and seen[1] == 7 and seen[2] is None and seen[3] is b and seen[4] == 2.5
    assert [what for what, _ in log] == ["on_device", "stream_ptr"] and all(dev is run.device for _, dev in log)
    res, added, lib = run(0)
    assert res is None and added == 1 and lib.seen == [(run.sentinel,)]


@pytest.mark.parametrize("code", [0, -1, -2, 3])
def test_launch_counts_once_or_not_at_all_whatever_the_code(stub, code):
    run, _ = stub
    assert run(code, 1)[1] == 1
    assert run(code, 1, count=False)[1] == 0
    assert run(code, 1, raw=True)[1] == 1
    assert run(code, 1, raw=True, count=False)[1] == 0
    assert run(code, 1, raw=True, count="ok")[1] == (1 if code >= 0 else 0)   # "ok": a call that declined launched nothing


@pytest.mark.parametrize("count", [1, 0, None, "OK", "yes"])
def test_launch_refuses_any_other_count_before_it_calls(stub, count):
    run, log = stub
    res, added, lib = run(0, 1, count=count)
    assert type(res) is ValueError and "count" in str(res) and added == 0 and not lib.seen and not log


def test_launch_checks_the_code(stub):
    run, _ = stub
    assert run(0, 1, what="thing")[0] is None
    err = run(-1, 1, what="thing")[0]
    assert type(err) is RuntimeError and str(err) == "thing: invalid argument"
    err = run(-1, 1)[0]
    assert type(err) is RuntimeError and str(err) == "ptb_fake: invalid argument"
    err = run(-2, 1, what="thing")[0]
    assert type(err) is NotImplementedError and str(err).startswith("thing: ")
    assert type(run(-2, 1)[0]) is NotImplementedError and str(run(-2, 1)[0]).startswith("ptb_fake: ")


@pytest.mark.parametrize("code", [-2, 0, 3])
def test_launch_raw_hands_the_code_back(stub, code):
    run, _ = stub
    res, added, lib = run(code, 5, raw=True, what="thing")
    assert res == code and type(res) is int and added == 1 and lib.seen == [(5, run.sentinel)]


def test_ptr():
    t = torch.arange(6, dtype=torch.float32)
    assert N.ptr(None) is None
    assert N.ptr(t) == t.data_ptr() and N.ptr(t[2:]) == t.data_ptr() + 8


def test_raw_stream_is_what_stream_ptr_asks(monkeypatch):
    asked = []
    monkeypatch.setattr(N, "raw_stream", lambda index: asked.append(index) or 0x1234)
    assert N.stream_ptr(torch.device("cuda", 3)).value == 0x1234 and asked == [3]
