"""CPU: the lockstep solver of the logistic-regression probe (sm3hip/logreg.py solver="lockstep", csrc/logreg.hip) -- what can be
said without a device: the tool's flag, the solver argument's refusal before any device call, the new entry points in header,
binding and library (ABI 9, additive), their refusals before any launch, the column table."""
import ctypes as C
import importlib.util
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
sys.path.insert(0, os.path.join(ROOT, "tests"))

ENTRY_POINTS = {"sm3_logreg_lockstep_slab": 0, "sm3_logreg_lockstep_workspace": 6, "sm3_logreg_batch_logits": 11,
                "sm3_logreg_batch_grad": 13, "sm3_logreg_value_grad_lockstep": 19, "sm3_logreg_fit_lockstep": 22}


def _tool():
    spec = importlib.util.spec_from_file_location("sm3_logreg_cli_lockstep_cpu", os.path.join(TOOLS, "backbone_logreg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _no_device(monkeypatch):
    for name in ("is_available", "synchronize", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, lambda *a: (_ for _ in ()).throw(AssertionError("the device was touched")))


def test_the_tool_accepts_and_refuses_solver_values(tmp_path, monkeypatch):
    tool = _tool()
    base = ["--data-name", "synthetic", "--data-path", "-"]
    p = tool.get_parser()
    assert p.parse_args(base).logreg_solver == "workgroup"
    for s in ("workgroup", "lockstep"):
        assert p.parse_args(base + ["--logreg-solver", s]).logreg_solver == s
    _no_device(monkeypatch)
    with pytest.raises(SystemExit, match="--logreg-solver newton is not one of workgroup, lockstep") as e:
        tool.main(base + ["-a", "resnet18", "--log-path", str(tmp_path), "-b", "8", "--logreg-solver", "newton"])
    assert e.value.code not in (0, None)
    spec = importlib.util.spec_from_file_location("sm3_logreg_bench_cpu", os.path.join(TOOLS, "logreg_bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.get_parser().parse_args([]).solver == "workgroup"
    assert bench.get_parser().parse_args(["--solver", "both"]).solver == "both"
    with pytest.raises(SystemExit):
        bench.get_parser().parse_args(["--solver", "newton"])


def test_an_unknown_solver_raises_before_any_device_call(monkeypatch):
    from sm3hip import logreg
    _no_device(monkeypatch)
    assert logreg.SOLVERS == ("workgroup", "lockstep")
    X, T = torch.zeros(6, 3), torch.zeros(6, 8, dtype=torch.long)
    T[:3] = 1
    with pytest.raises(ValueError, match="solver"):
        logreg.fit(X, T, [1.0], solver="newton")
    with pytest.raises(ValueError, match="solver"):
        logreg.fit_problems(X, T, [(0, 1.0, 0)], solver="newton")
    with pytest.raises(ValueError, match="solver"):
        logreg.value_and_grad(X, T, [(0, 1.0, 0)], torch.zeros(1, 5, 3), torch.zeros(1, 5), solver="newton")
    for s in logreg.SOLVERS:                                                       # a known solver gets as far as the device check
        with pytest.raises(ValueError, match="GPU"):
            logreg.fit(X, T, [1.0], solver=s)
        with pytest.raises(ValueError, match="GPU"):
            logreg.value_and_grad(X, T, [(0, 1.0, 0)], torch.zeros(1, 5, 3), torch.zeros(1, 5), solver=s)


def test_header_binding_and_library_carry_the_new_entry_points():
    from sm3hip import _lib, logreg, ops
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sm3_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        declared = 0 if m.group(1).strip() == "void" else len(m.group(1).split(","))
        assert declared == len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name)
    assert lib.sm3_abi_version() == 9
    assert lib.sm3_logreg_lockstep_slab() == ops.LOGREG_LOCKSTEP_SLAB == 2048
    # per problem the workgroup fit's vectors and rows and 24 words of state; per column one row of D per slab; the modes
    nvec, N, D = 8 * 3 + 8, 10, 3
    assert ops.logreg_lockstep_workspace(N, D, 2, 7, True) == 2 * (23 * nvec + 3 * N * 8 + 24) + 1 * 7 * D + 1
    assert ops.logreg_lockstep_workspace(2049, D, 3, 8, False) == 3 * (2 * 2049 * 8 + 2) + 2 * 8 * D + 2
    assert ops.logreg_columns([2, 3]).tolist() == [0, 1, 8, 9, 10]
    assert logreg.lockstep_chunk(N, D, 5) == 5 and logreg.lockstep_chunk(16384, 4096, 10 ** 6) >= 64
    # the values the workgroup solver's callers rely on stay
    assert ops.logreg_workspace(10, 3, True) == 23 * nvec + 3 * 10 * 8 + 16 and logreg.default_chunk(10, 3, 7) == 7
    assert logreg.launch_iterations(10, 3) == 32 and logreg.launch_iterations(16384, 4096) == 4


def test_the_new_entry_points_reject_bad_arguments_before_any_launch():
    from sm3hip import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 4096)()
    p = C.cast(buf, C.c_void_p)  # host memory: never dereferenced by a kernel, every call below returns before a launch
    odd, odd2 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 2)
    big = 1 << 40
    fit = lambda X=p, t=p, w=p, tab=p, Cs=p, cols=p, N=5, D=3, R=1, P=2, nc=4, gtol=1e-9, it=10, resume=0, iters=4, ws=p, n=big, coef=p, \
        icpt=p, info=p, res=p: lib.sm3_logreg_fit_lockstep(X, t, w, tab, Cs, cols, N, D, R, P, nc, gtol, it, resume, iters, ws, n, coef,
                                                           icpt, info, res, None)
    vg = lambda X=p, t=p, w=p, tab=p, Cs=p, cols=p, W=p, b=p, N=5, D=3, R=1, P=2, nc=4, ws=p, n=big, F=p, gW=p, gb=p: \
        lib.sm3_logreg_value_grad_lockstep(X, t, w, tab, Cs, cols, W, b, N, D, R, P, nc, ws, n, F, gW, gb, None)
    lg = lambda X=p, V=p, cols=p, act=p, N=5, D=3, P=2, nc=4, Z=p: lib.sm3_logreg_batch_logits(X, V, None, cols, act, N, D, P, nc, Z, None)
    gr = lambda X=p, Rm=p, cols=p, act=p, N=5, D=3, P=2, nc=4, ws=p, n=big, G=p, gb=p: \
        lib.sm3_logreg_batch_grad(X, Rm, cols, act, N, D, P, nc, ws, n, G, gb, None)
    for call, pointers in ((fit, ("X", "t", "w", "tab", "Cs", "cols", "ws", "coef", "icpt", "info", "res")),
                           (vg, ("X", "t", "w", "tab", "Cs", "cols", "W", "b", "ws", "F", "gW", "gb")),
                           (lg, ("X", "V", "cols", "act", "Z")), (gr, ("X", "Rm", "cols", "act", "ws", "G", "gb"))):
        for arg in pointers:
            assert call(**{arg: None}) == -1, arg
        assert call(D=0) == -1 and call(D=4097) == -1 and call(P=0) == -1 and call(P=65536) == -1
        assert call(nc=0) == -1 and call(nc=17) == -1                              # more columns than 8 P
        for N in (0, -1, 16385):
            assert call(N=N) == -1
        assert call(X=odd2) == -2 and call(cols=odd2) == -2
    for call in (fit, vg):
        assert call(R=0) == -1 and call(n=10) == -1                               # a workspace that is too small
        assert call(w=odd) == -2 and call(ws=odd) == -2 and call(tab=odd2) == -2
    assert gr(n=1 * 4 * 3 - 1) == -1 and gr(N=2049, n=2 * 4 * 3 - 1) == -1         # slabs * columns * D elements are needed
    assert gr(ws=odd) == -2 and gr(G=odd) == -2
    assert lg(Z=odd) == -2 and lg(V=odd) == -2 and lg(act=odd2) == -2
    assert lib.sm3_logreg_batch_logits(p, p, odd, p, p, 5, 3, 2, 4, p, None) == -2  # the optional intercepts
    assert fit(gtol=-1.0) == -1 and fit(gtol=float("nan")) == -1 and fit(gtol=float("inf")) == -1 and fit(it=-1) == -1
    assert fit(iters=0) == -1 and fit(iters=1025) == -1 and fit(resume=2) == -1 and fit(resume=-1) == -1
    assert fit(coef=odd) == -2 and fit(info=odd2) == -2 and vg(gW=odd) == -2 and vg(F=odd) == -2
    out = C.c_int64(0)
    wsf = lib.sm3_logreg_lockstep_workspace
    assert wsf(5, 3, 2, 4, 1, C.byref(out)) == 0 and out.value > 0
    for bad in ((0, 3, 2, 4), (16385, 3, 2, 4), (5, 0, 2, 4), (5, 4097, 2, 4), (5, 3, 0, 1), (5, 3, 65536, 4), (5, 3, 2, 0), (5, 3, 2, 17)):
        assert wsf(*bad, 1, C.byref(out)) == -1, bad
    assert wsf(5, 3, 2, 4, 1, None) == -1
