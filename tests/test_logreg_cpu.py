"""CPU: the logistic-regression probe (sm3hip/logreg.py, csrc/logreg.hip, tools/backbone_logreg.py) -- what can be said without
a device.

  * the fp64 numpy restatement (tests/logreg_inputs.py) is pinned to scikit-learn: on every problem the GPU tests fit (SHAPES x
    LABELS x weight rows x C in {0.01, 1, 100}) its held-out probabilities agree with LogisticRegression(C, or 2 C where two
    classes remain, sample_weight=s) within PARITY_BOUND[C] = 4 x the gap measured with scikit-learn 1.7.2 and recorded in
    logreg_inputs.MEASURED_GAP; so do class_weight="balanced", a 0/1 fold row, an integer multiplicity row (which also equals
    the fit on physically repeated rows) and a class of zero weight (scikit-learn on the reduced label set);
  * it converges (status ok, fewer than 1000 iterations) on every one of those problems;
  * its gradient is the central difference of its objective;
  * folds are a partition, fractions are nested and keep every present class, pick breaks ties towards the smaller C,
    to_baseline_state folds "standardize" into the heads and refuses "l2";
  * the tool's parser accepts backbone_knn's line and every refusal fires before the device is touched;
  * header, binding and library carry the entry points (ABI 9), which refuse bad arguments before any launch."""
import ctypes as C
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import logreg_inputs as L  # noqa: E402

ENTRY_POINTS = {"sm3_logreg_max_rows": 0, "sm3_logreg_workspace": 4, "sm3_logreg_check_host": 8, "sm3_logreg_value_grad": 17,
                "sm3_logreg_fit": 20, "sm3_logreg_predict": 9}


# ---- the restatement against scikit-learn -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", L.SHAPES)
def test_restatement_matches_scikit_learn_and_converges(shape):
    N, D = shape
    X, T, Xq = L.make_case(N, D)
    rows, ref = L.case_rows(N, T), L.reference(N, D)
    worst = {c: 0.0 for c in L.PARITY_CS}
    for (t, r, c), f in ref.items():
        nt, s = L.NUM_CLASSES[t], rows[r]
        assert f["status"] == "ok" and f["iterations"] < 1000 and f["grad_norm"] <= 1e-10, (shape, t, r, c, f["status"], f["grad_norm"])
        gap = np.abs(f["probs"] - L.sklearn_probs(X, T[:, t], s, c, nt, Xq)).max()
        worst[c] = max(worst[c], gap)
        assert gap <= L.PARITY_BOUND[c], (shape, L.ROW_KINDS[r], t, c, gap)
        pres = L.present_classes(T[:, t], s, nt)
        assert not f["probs"][:, ~pres].any() and not f["W"][~pres].any()
    print(f"N {N} D {D}: worst probability gap to scikit-learn " + ", ".join(f"C {c}: {g:.2e}" for c, g in worst.items()))


@pytest.mark.parametrize("shape", ((17, 33), (65, 130)))
def test_restatement_balanced_and_repeated_rows(shape):
    N, D = shape
    X, T, Xq = L.make_case(N, D)
    rows = L.case_rows(N, T)
    for t in L.LABELS:
        nt, y = L.NUM_CLASSES[t], T[:, t]
        for c in L.PARITY_CS:
            f = L.fit_ref(X, y, L.balanced(rows[1], y, nt), c, nt)               # balanced on top of the fold row
            gap = np.abs(L.probs(f["W"], f["b"], Xq) - L.sklearn_probs(X, y, rows[1], c, nt, Xq, class_weight="balanced")).max()
            assert f["status"] == "ok" and gap <= L.PARITY_BOUND[c], ("balanced", shape, t, c, gap)
            rep = np.repeat(np.arange(N), rows[2].astype(np.int64))               # multiplicities = repeated rows
            g = L.fit_ref(X[rep], y[rep], np.ones(len(rep)), c, nt)
            m = L.reference(N, D)[(t, 2, c)]
            gap = np.abs(L.probs(g["W"], g["b"], Xq) - m["probs"]).max()
            assert g["status"] == "ok" and gap <= L.PARITY_BOUND[c], ("repeated", shape, t, c, gap)
    s = rows[3]
    assert (L.present_classes(T[:, 1], s, 3) == [True, False, True]).all()       # the row that takes PN's class 1 away
    one = rows[0].copy()
    one[T[:, 2] == 1] = 0.0
    assert L.fit_ref(X, T[:, 2], one, 1.0, 2)["status"] == "one_class"


def test_measured_gaps_are_recorded():
    """The recorded figure is the measured one: the measurement is repeated here -- every problem of every shape, plain and with
    class_weight="balanced" on the fold row -- and its worst gap per C lies within a factor 2 of the record (scikit-learn's
    stopping point moves a little with the BLAS and the thread count) and, as every parity test asserts, within the bound."""
    assert L.PARITY_BOUND == {c: 4.0 * g for c, g in L.MEASURED_GAP.items()} and set(L.MEASURED_GAP) == set(L.PARITY_CS)
    worst = {c: 0.0 for c in L.PARITY_CS}
    for (N, D) in L.SHAPES:
        X, T, Xq = L.make_case(N, D)
        rows = L.case_rows(N, T)
        for (t, r, c), f in L.reference(N, D).items():
            worst[c] = max(worst[c], np.abs(f["probs"] - L.sklearn_probs(X, T[:, t], rows[r], c, L.NUM_CLASSES[t], Xq)).max())
        for t in L.LABELS:
            nt, y = L.NUM_CLASSES[t], T[:, t]
            for c in L.PARITY_CS:
                f = L.fit_ref(X, y, L.balanced(rows[1], y, nt), c, nt)
                ps = L.sklearn_probs(X, y, rows[1], c, nt, Xq, class_weight="balanced")
                worst[c] = max(worst[c], np.abs(L.probs(f["W"], f["b"], Xq) - ps).max())
    for c in L.PARITY_CS:
        print(f"C {c}: worst gap seen {worst[c]:.3e}, recorded {L.MEASURED_GAP[c]:.3e}")
        assert L.MEASURED_GAP[c] / 2.0 <= worst[c] <= min(2.0 * L.MEASURED_GAP[c], L.PARITY_BOUND[c]), (c, worst[c])


def test_library_balanced_weights_are_the_restatement_s():
    from sm3hip import logreg
    for (N, D) in ((17, 33), (65, 130)):
        _, T, _ = L.make_case(N, D)
        rows = L.case_rows(N, T)
        for t in range(8):
            got = logreg.balanced(torch.from_numpy(rows), torch.from_numpy(T), t).numpy()
            for r in range(rows.shape[0]):
                want = L.balanced(rows[r], T[:, t], L.NUM_CLASSES[t])
                assert np.abs(got[r] - want).max() <= 4 * 2.0 ** -53 * want.max(), (N, t, r)


def test_gradient_is_the_central_difference_of_the_objective():
    rs = np.random.RandomState(0)
    for (N, D) in ((3, 5), (17, 33)):
        X, T, _ = L.make_case(N, D)
        rows = L.case_rows(N, T)
        for t in L.LABELS:
            nt = L.NUM_CLASSES[t]
            for r in (0, 2, 3):
                W, b = rs.randn(nt, D) * 0.3, rs.randn(nt) * 0.3
                pres = L.present_classes(T[:, t], rows[r], nt)
                F, gW, gb = L.value_and_grad(X, T[:, t], rows[r], 0.7, W, b, nt)
                h = 1e-6
                for _ in range(6):
                    c, k = rs.randint(nt), rs.randint(D)
                    Wp, Wm = W.copy(), W.copy()
                    Wp[c, k] += h
                    Wm[c, k] -= h
                    num = (L.value_and_grad(X, T[:, t], rows[r], 0.7, Wp, b, nt)[0]
                           - L.value_and_grad(X, T[:, t], rows[r], 0.7, Wm, b, nt)[0]) / (2 * h)
                    assert abs(num - gW[c, k]) <= 1e-8 * max(1.0, abs(num)), (N, D, t, r, c, k)
                    bp, bm = b.copy(), b.copy()
                    bp[c] += h
                    bm[c] -= h
                    num = (L.value_and_grad(X, T[:, t], rows[r], 0.7, W, bp, nt)[0]
                           - L.value_and_grad(X, T[:, t], rows[r], 0.7, W, bm, nt)[0]) / (2 * h)
                    assert abs(num - gb[c]) <= 1e-8 * max(1.0, abs(num))
                assert not gb[~pres].any() and abs(gb.sum()) < 1e-15


# ---- host-side functions ------------------------------------------------------------------------------------------------
def test_folds_are_a_partition():
    from sm3hip import logreg
    for N, K, seed in ((7, 3, 0), (100, 5, 1), (413, 10, 2 ** 63 + 5), (4, 4, 0)):
        rows = logreg.folds(N, K, seed)
        assert tuple(rows.shape) == (K, N) and rows.dtype == torch.float64 and set(rows.unique().tolist()) <= {0.0, 1.0}
        held = rows == 0
        assert bool((held.sum(dim=0) == 1).all())                                  # every case is held out exactly once
        sizes = held.sum(dim=1)
        assert int(sizes.max() - sizes.min()) <= 1
        assert torch.equal(rows, logreg.folds(N, K, seed))
    assert not torch.equal(logreg.folds(100, 5, 1), logreg.folds(100, 5, 2))
    for bad in ((5, 1, 0), (5, 6, 0), (5, 2, -1), (5, 2.0, 0)):
        with pytest.raises(ValueError):
            logreg.folds(*bad)


def test_fractions_are_nested_and_keep_every_class():
    from sm3hip import logreg
    rs = np.random.RandomState(0)
    N = 413
    T = np.stack([rs.randint(0, n, N) for n in L.NUM_CLASSES], axis=1)
    T[:, 0] = np.where(rs.rand(N) < 0.01, 4, T[:, 0] % 4)                        # a rare class
    fr = (0.01, 0.1, 0.5, 1.0)
    rows = logreg.fractions(torch.from_numpy(T), fr, 3).numpy()
    assert rows.shape == (4, N) and rows[3].all()
    for a in range(3):
        assert ((rows[a] == 1) <= (rows[a + 1] == 1)).all()                        # nested
    for r, f in enumerate(fr):
        assert int(rows[r].sum()) >= int(np.ceil(f * N)) and int(rows[r].sum()) <= max(int(np.ceil(f * N)), 24)
        for t, n in enumerate(L.NUM_CLASSES):
            assert set(np.unique(T[rows[r] == 1, t])) == set(np.unique(T[:, t]))   # every class that is present stays
    assert np.array_equal(rows, logreg.fractions(torch.from_numpy(T), fr, 3).numpy())
    for bad in ((0.0,), (1.5,), ()):
        with pytest.raises(ValueError, match="fraction"):
            logreg.fractions(torch.from_numpy(T), bad, 0)


def test_pick_breaks_ties_towards_the_smaller_c():
    from sm3hip import logreg
    Cs = [100.0, 0.01, 1.0]
    table = [[0.7, 0.7, 0.7], [0.9, 0.5, 0.9], [0.1, 0.2, 0.3]]
    assert logreg.pick(table, Cs) == [0.01, 1.0, 1.0]
    assert logreg.pick(table, Cs, per_label=False) == [1.0, 1.0, 1.0]             # means 0.567, 0.467, 0.633
    assert logreg.pick([[0.5, 0.5, 0.5]] * 2, Cs, per_label=False) == [0.01, 0.01]


def _host_fit(D, seed=0):
    from sm3hip import logreg
    rs = np.random.RandomState(seed)
    problems = [(t, 1.0, 0) for t in range(8)]
    coef, icpt = torch.zeros(8, 5, D, dtype=torch.float64), torch.zeros(8, 5, dtype=torch.float64)
    for t, n in enumerate(L.NUM_CLASSES):
        coef[t, :n], icpt[t, :n] = torch.from_numpy(rs.randn(n, D)), torch.from_numpy(rs.randn(n))
    return logreg.Fit(coef=coef, intercept=icpt, problems=problems, n_classes=list(L.NUM_CLASSES), labels=list(range(8)), Cs=[1.0])


def test_to_baseline_state_folds_standardize_and_refuses_l2():
    from sm3hip import logreg
    from src.models.baseline import Baseline
    D = 1024
    rs = np.random.RandomState(1)
    X = torch.from_numpy((rs.randn(50, D) * 2.0 + 3.0).astype(np.float32))
    X[:, 7] = 1.25                                                                 # a constant feature: only centred
    norm = logreg.normalize_fit(X, "standardize")
    Xn = logreg.normalize_apply(X, norm)
    assert Xn.dtype == torch.float32 and float(Xn.double().mean(dim=0).abs().max()) < 1e-6 and not Xn[:, 7].any()
    assert float((Xn.double().std(dim=0, unbiased=False)[:7] - 1).abs().max()) < 1e-6
    fit = _host_fit(D)
    which = list(range(8))
    state = logreg.to_baseline_state(fit, which, norm)
    model = Baseline("resnet18", None)
    missing = model.load_state_dict(state, strict=False)
    assert not missing.unexpected_keys and all(not k.startswith("classifier") for k in missing.missing_keys)
    for t, n in enumerate(L.NUM_CLASSES):
        want = Xn.double() @ fit.coef[t, :n].T + fit.intercept[t, :n]
        got = model.classifier[t](X).double().detach()
        w = state[f"classifier.{t}.weight"].double().abs()
        tol = 4 * (D + 2) * 2.0 ** -24 * float((w @ X.double().abs().T).max() + 1)   # fp32 rounding of a D-term dot product
        assert float((got - want).abs().max()) <= tol, (t, float((got - want).abs().max()), tol)
    none = logreg.to_baseline_state(fit, which, logreg.normalize_fit(X, "none"))
    assert torch.equal(none["classifier.0.weight"], fit.coef[0, :5].float())
    with pytest.raises(ValueError, match="l2"):
        logreg.to_baseline_state(fit, which, logreg.normalize_fit(X, "l2"))
    with pytest.raises(ValueError, match="one problem per label"):
        logreg.to_baseline_state(fit, which[::-1], norm)
    with pytest.raises(ValueError, match="kind"):
        logreg.normalize_fit(X, "whiten")


def test_library_refusals_with_no_device():
    from sm3hip import logreg
    X, T = torch.zeros(6, 3), torch.zeros(6, 8, dtype=torch.long)
    T[:3] = 1
    with pytest.raises(ValueError, match="float32"):
        logreg.fit(X.double(), T)
    with pytest.raises(ValueError, match="targets"):
        logreg.fit(X, T[:, :7])
    with pytest.raises(ValueError, match="weights"):
        logreg.fit(X, T, weights=torch.ones(2, 5))
    with pytest.raises(ValueError, match="class_weight"):
        logreg.fit(X, T, class_weight="sqrt")
    with pytest.raises(ValueError, match="labels"):
        logreg.fit(X, T, labels=[0, 0])
    with pytest.raises(ValueError, match="chunk"):
        logreg.fit(X, T, chunk=0)
    bad = T.clone()
    bad[0, 2] = 2                                                                  # BWV has two classes
    for kw in (dict(targets=bad), dict(weights=-torch.ones(1, 6)), dict(weights=torch.full((1, 6), float("inf"))),
               dict(Cs=[0.0]), dict(Cs=[float("nan")])):
        with pytest.raises(ValueError, match="logreg"):
            logreg.fit(X, **{**dict(targets=T, Cs=[1.0]), **kw})
    with pytest.raises(ValueError, match="GPU"):                                   # everything else is fine: only the device is not
        logreg.fit(X, T, [1.0])
    with pytest.raises(ValueError, match="GPU"):
        logreg.value_and_grad(X, T, [(0, 1.0, 0)], torch.zeros(1, 5, 3), torch.zeros(1, 5))
    with pytest.raises(ValueError, match="widest label"):
        logreg.value_and_grad(X, T, [(0, 1.0, 0)], torch.zeros(1, 3, 3), torch.zeros(1, 3))
    assert len(logreg.DEFAULT_CS) == 16 and abs(logreg.DEFAULT_CS[0] - 1e-4) < 1e-19 and abs(logreg.DEFAULT_CS[-1] - 1e4) < 1e-9


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_carry_the_entry_points():
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
    assert lib.sm3_logreg_max_rows() == logreg.MAX_ROWS == ops.LOGREG_MAX_ROWS == 16384 and ops.LOGREG_MAX_DIM == 4096
    assert ops.logreg_workspace(10, 3, True) == 23 * (8 * 3 + 8) + 3 * 10 * 8 + 16 and ops.logreg_workspace(10, 3, False) == 160


def test_entry_points_reject_bad_arguments_before_any_launch():
    from sm3hip import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 4096)()
    p = C.cast(buf, C.c_void_p)  # host memory: never dereferenced by a kernel, every call below returns before a launch
    odd, odd2 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 2)
    big = 1 << 40
    fit = lambda X=p, t=p, w=p, tab=p, Cs=p, N=5, D=3, R=1, P=2, gtol=1e-9, it=10, resume=0, iters=4, ws=p, n=big, coef=p, icpt=p, info=p, \
        res=p: lib.sm3_logreg_fit(X, t, w, tab, Cs, N, D, R, P, gtol, it, resume, iters, ws, n, coef, icpt, info, res, None)
    vg = lambda X=p, t=p, w=p, tab=p, Cs=p, W=p, b=p, N=5, D=3, R=1, P=2, ws=p, n=big, F=p, gW=p, gb=p: \
        lib.sm3_logreg_value_grad(X, t, w, tab, Cs, W, b, N, D, R, P, ws, n, F, gW, gb, None)
    pr = lambda Xq=p, coef=p, icpt=p, nts=p, Q=5, D=3, P=2, out=p: lib.sm3_logreg_predict(Xq, coef, icpt, nts, Q, D, P, out, None)
    for call, pointers in ((fit, ("X", "t", "w", "tab", "Cs", "ws", "coef", "icpt", "info", "res")),
                           (vg, ("X", "t", "w", "tab", "Cs", "W", "b", "ws", "F", "gW", "gb")),
                           (pr, ("Xq", "coef", "icpt", "nts", "out"))):
        for arg in pointers:
            assert call(**{arg: None}) == -1, arg
        assert call(D=0) == -1 and call(D=4097) == -1 and call(P=0) == -1
    for call in (fit, vg):
        for N in (0, -1, 16385):
            assert call(N=N) == -1
        assert call(R=0) == -1 and call(n=10) == -1                               # a workspace that is too small
        assert call(X=odd2) == -2 and call(w=odd) == -2 and call(ws=odd) == -2 and call(tab=odd2) == -2
    assert fit(gtol=-1.0) == -1 and fit(gtol=float("nan")) == -1 and fit(gtol=float("inf")) == -1 and fit(it=-1) == -1
    assert fit(iters=0) == -1 and fit(resume=2) == -1 and fit(resume=-1) == -1
    assert fit(coef=odd) == -2 and fit(info=odd2) == -2 and vg(gW=odd) == -2 and vg(F=odd) == -2
    assert pr(Q=0) == -1 and pr(Q=(1 << 24) + 1) == -1 and pr(P=65536) == -1 and pr(out=odd) == -2 and pr(Xq=odd2) == -2
    out = C.c_int64(0)
    assert lib.sm3_logreg_workspace(0, 3, 1, C.byref(out)) == -1 and lib.sm3_logreg_workspace(5, 3, 1, None) == -1
    # the host check of the problem data: class indices, weights, C, the table
    N, R, P = 4, 2, 2
    ncls = (C.c_int32 * 8)(*L.NUM_CLASSES)
    def check(targets=None, weights=None, table=None, Cs=None, n=N, r=R, pp=P):
        t = (C.c_int32 * (N * 8))(*([0, 1] * (N * 4)) if targets is None else targets)
        w = (C.c_double * (R * N))(*([1.0, 0.0] * N if weights is None else weights))
        tb = (C.c_int32 * (P * 4))(*([0, 0, 5, 0, 2, 1, 2, 0] if table is None else table))
        cs = (C.c_double * P)(*([1.0, 0.5] if Cs is None else Cs))
        return lib.sm3_logreg_check_host(t, w, tb, cs, ncls, n, r, pp)
    assert check() == 0
    assert check(targets=[5] + [0] * 31) == -1 and check(targets=[-1] + [0] * 31) == -1     # label 0 has 5 classes
    assert check(targets=[0, 3] + [0] * 30) == 0                                            # label 1 is not fitted: not read
    assert check(targets=[0, 0, 2] + [0] * 29) == -1                                        # label 2 has 2 classes
    assert check(weights=[-1.0] + [1.0] * 7) == -1 and check(weights=[float("nan")] + [1.0] * 7) == -1
    assert check(weights=[float("inf")] + [1.0] * 7) == -1
    for bad in ([0.0, 1.0], [-1.0, 1.0], [float("inf"), 1.0], [float("nan"), 1.0]):
        assert check(Cs=bad) == -1
    assert check(table=[8, 0, 5, 0, 2, 1, 2, 0]) == -1 and check(table=[0, 2, 5, 0, 2, 1, 2, 0]) == -1
    assert check(table=[0, 0, 3, 0, 2, 1, 2, 0]) == -1                                      # n_t that is not the label's
    assert check(n=0) == -1 and check(n=16385) == -1 and check(r=0) == -1 and check(pp=0) == -1


# ---- the tool -----------------------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("sm3_logreg_cli_cpu", os.path.join(TOOLS, "backbone_logreg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_backbone_logreg_parses_its_flags():
    p = _tool().get_parser()
    base = ["--data-name", "synthetic", "--data-path", "-"]
    d = p.parse_args(base)
    assert len(d.logreg_c) == 16 and abs(d.logreg_c[0] - 1e-4) < 1e-18 and abs(d.logreg_c[-1] - 1e4) < 1e-9
    assert (d.logreg_select, d.logreg_folds, d.logreg_by, d.logreg_shared_c) == ("val", 5, "auc", False)
    assert (d.logreg_fractions, d.logreg_class_weight, d.logreg_normalize) == ([1.0], "none", "standardize")
    assert (d.logreg_gtol, d.logreg_max_iter, d.save_features, d.random_features) == (1e-9, 1000, False, None)
    a = p.parse_args(base + ["-a", "resnet50", "--mean", "0.7833", "0.6712", "0.6026", "--std", "0.2139", "0.2472", "0.2571",
                             "-b", "128", "-j", "4", "--img-sz", "224", "224", "--pretrain-path", "logs/ckp_399.pth", "--log-path",
                             "logs/knn", "--bootstrap", "2000", "--calibration", "--operating", "--checklist",   # backbone_knn's line
                             "--logreg-c", "0.1", "10", "--logreg-select", "cv", "--logreg-folds", "4", "--logreg-by", "nll",
                             "--logreg-shared-c", "--logreg-fractions", "0.01", "0.1", "1", "--logreg-class-weight", "balanced",
                             "--logreg-normalize", "l2", "--logreg-gtol", "1e-8", "--logreg-max-iter", "50", "--save-features",
                             "--random-features", "96", "40", "64"])
    assert a.logreg_c == [0.1, 10.0] and (a.logreg_select, a.logreg_folds, a.logreg_by, a.logreg_shared_c) == ("cv", 4, "nll", True)
    assert a.logreg_fractions == [0.01, 0.1, 1.0] and (a.logreg_class_weight, a.logreg_normalize) == ("balanced", "l2")
    assert (a.logreg_gtol, a.logreg_max_iter, a.save_features, a.random_features) == (1e-8, 50, True, [96, 40, 64])
    assert a.bootstrap == 2000 and a.calibration and a.operating and a.checklist and a.arch == "resnet50"


def test_backbone_logreg_refuses_before_the_device_is_touched(tmp_path, monkeypatch):
    tool = _tool()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("the device was touched")))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: (_ for _ in ()).throw(AssertionError("the device was touched")))
    syn = ["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "--log-path", str(tmp_path), "-b", "8"]
    for extra, text in ((["--logreg-select", "loo"], "--logreg-select loo is not one of"),
                        (["--logreg-by", "acc"], "--logreg-by acc is not one of"),
                        (["--logreg-class-weight", "sqrt"], "--logreg-class-weight sqrt is not one of"),
                        (["--logreg-normalize", "whiten"], "--logreg-normalize whiten is not one of"),
                        (["--logreg-select", "cv", "--logreg-folds", "1"], "K >= 2"),
                        (["--logreg-fractions", "0"], r"\(0, 1\]"), (["--logreg-fractions", "0.5", "1.5"], r"\(0, 1\]"),
                        (["--logreg-select", "cv", "--logreg-fractions", "0.5"], "must be 1"),
                        (["--logreg-c", "0"], "positive and finite"), (["--logreg-c", "1", "1"], "twice"),
                        (["--logreg-select", "none"], "exactly one"), (["--logreg-refit-trainval", "--logreg-select", "cv"], "goes with"),
                        (["--logreg-gtol", "-1"], "gtol"), (["--logreg-max-iter", "0"], "max-iter"),
                        (["--random-features", "20000", "4", "8"], "at most"), (["--random-features", "0", "4", "8"], ">= 1"),
                        (["--steps-per-epoch", "4000"], "train rows")):
        with pytest.raises(SystemExit, match=text) as e:
            tool.main(syn + extra)
        assert e.value.code not in (0, None), extra
    with pytest.raises(SystemExit, match="plain ResNets"):
        tool.main(["--data-name", "synthetic", "--data-path", "-", "-a", "resnext50_32x4d", "--log-path", str(tmp_path)])
    import shutil
    meta = os.path.join(ROOT, "tests", "golden", "derm7pt_meta")                   # a derm7pt tree without its images
    tree = tmp_path / "7PC"
    os.makedirs(tree / "images")
    for f in ("meta.csv", "train_indexes.csv", "valid_indexes.csv", "test_indexes.csv"):
        shutil.copy(os.path.join(meta, f), tree / f)
    with pytest.raises(SystemExit, match="--random-features goes with --data-name synthetic"):
        tool.main(["--data-name", "SevenPCBaseDataset", "--data-path", str(tree), "-a", "resnet18", "--log-path", str(tmp_path),
                   "--random-features", "96", "40", "64"])
