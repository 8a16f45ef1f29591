"""GPU: the logistic-regression probe (csrc/logreg.hip, sm3hip/logreg.py, tools/backbone_logreg.py) against the fp64 numpy
restatement of tests/logreg_inputs.py, which tests/test_logreg_cpu.py pins to scikit-learn.  The reference is never the code
under test.  Shapes: N in {2, 3, 17, 65, 130}, D in {1, 5, 33, 130, 515} (and D = 1030 for value_and_grad: the second sweep of
the gradient's feature loop), labels of 2, 3 and 5 classes, 1 to 37 problems a call, weight rows that hold zeros.

  * value_and_grad: F and every gradient entry within logreg_inputs.value_grad_bound (derived there: the two sides differ in the
    ORDER of fp64 sums over N and D terms, nothing else), on random inputs and on integer-valued X, W, b scaled by powers of two,
    where the logits are exact and only the softmax rounds;
  * the certificate: at every returned (W, b) of status ok the restatement's |grad F|_inf is <= gtol + that bound;
  * the optimum: held-out probabilities within logreg_inputs.PARITY_BOUND[C] of the restatement's optimum;
  * weights: a multiplicity row = the fit on repeated rows (same bound); a class without weight has probability 0 and coefficient
    row 0; a problem with one class returns its status and leaves the rest of the batch bit-unchanged;
  * bits: alone = in a batch of 37 at the first and the last position; chunk 1 = 5 = all; two calls; predict row by row = all rows;
  * every output in a sentinel-filled buffer whose other bytes stay; every refusal with no launch; the tool end to end."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import logreg_inputs as L  # noqa: E402

pytestmark = pytest.mark.gpu
GTOL = 1e-9


def _dev():
    return torch.device("cuda", 0)


def _case(N, D):
    X, T, Xq = L.make_case(N, D)
    return X, T, Xq, L.case_rows(N, T)


_FITS = {}


def fitted(N, D):
    """The grid fit of shape (N, D) (LABELS x rows_of x PARITY_CS), once a session."""
    from sm3hip import logreg
    if (N, D) not in _FITS:
        X, T, Xq, rows = _case(N, D)
        f = logreg.fit(torch.from_numpy(X).to(_dev()), torch.from_numpy(T), L.PARITY_CS, weights=torch.from_numpy(rows[list(L.rows_of((N, D)))]),
                       labels=L.LABELS, gtol=GTOL)
        _FITS[(N, D)] = f
    return _FITS[(N, D)]


def _probs(fit, p, Xq):
    from sm3hip import logreg
    nt = fit.n_classes[p]
    z = logreg.predict_all(fit, torch.from_numpy(Xq).to(_dev()), [p])[0, :, :nt]
    return torch.softmax(z, dim=1).cpu().numpy()


# ---- value and gradient -------------------------------------------------------------------------------------------------
def _check_value_grad(X, T, rows, W, b, Cs, tag):
    from sm3hip import logreg
    problems = [(t, Cs[(t + r) % len(Cs)], r) for t in L.LABELS for r in range(rows.shape[0])]
    P, D = len(problems), X.shape[1]
    Wp, bp = np.zeros((P, 5, D)), np.zeros((P, 5))
    for p, (t, _, _) in enumerate(problems):
        nt = L.NUM_CLASSES[t]
        Wp[p, :nt], bp[p, :nt] = W[p % len(W), :nt], b[p % len(b), :nt]
    F, gW, gb = logreg.value_and_grad(torch.from_numpy(X).to(_dev()), torch.from_numpy(T), problems, torch.from_numpy(Wp),
                                      torch.from_numpy(bp), weights=torch.from_numpy(rows))
    F, gW, gb = F.cpu().numpy(), gW.cpu().numpy(), gb.cpu().numpy()
    for p, (t, c, r) in enumerate(problems):
        nt = L.NUM_CLASSES[t]
        Fr, gWr, gbr = L.value_and_grad(X, T[:, t], rows[r], c, Wp[p], bp[p], nt)
        bF, bG = L.value_grad_bound(X, rows[r], c, Wp[p], bp[p], nt)
        dF, dW, db = abs(F[p] - Fr), np.abs(gW[p, :nt] - gWr).max(), np.abs(gb[p, :nt] - gbr).max()
        print(f"{tag} N {X.shape[0]} D {D} label {t} row {r} C {c}: |dF| {dF:.2e} (<= {bF:.2e}) |dgrad| {max(dW, db):.2e} (<= {bG:.2e})")
        assert dF <= bF and dW <= bG and db <= bG, (tag, p, dF, bF, dW, db, bG)
        assert not gW[p, nt:].any() and not gb[p, nt:].any()


@pytest.mark.parametrize("shape", L.SHAPES + ((17, 1030),))
def test_value_and_grad_against_the_restatement(shape):
    N, D = shape
    X, T, _, rows = _case(N, D)
    rs = np.random.RandomState(5)
    W, b = rs.randn(3, 5, D) / np.sqrt(D), rs.randn(3, 5)
    _check_value_grad(X, T, rows[[0, 2]], W, b, (0.01, 1.0, 100.0), "random")


@pytest.mark.parametrize("shape", ((3, 5), (65, 130), (17, 515)))
def test_value_and_grad_on_integer_inputs(shape):
    """X integers in [-3, 3], W integers / 16, b integers / 4: every logit is an exact fp64 number in any order."""
    N, D = shape
    _, T, _, rows = _case(N, D)
    rs = np.random.RandomState(6)
    X = rs.randint(-3, 4, (N, D)).astype(np.float32)
    W, b = rs.randint(-4, 5, (2, 5, D)) / 16.0, rs.randint(-8, 9, (2, 5)) / 4.0
    _check_value_grad(X, T, rows[[0, 2]], W, b, (0.5, 2.0), "integer")


# ---- the fit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", L.SHAPES)
def test_fit_certificate_and_optimum(shape):
    N, D = shape
    X, T, Xq, rows = _case(N, D)
    fit, ref = fitted(N, D), L.reference(N, D)
    status, iters = fit.status.cpu().numpy(), fit.iterations.cpu().numpy()
    coef, icpt, gn = fit.coef.cpu().numpy(), fit.intercept.cpu().numpy(), fit.grad_norm.cpu().numpy()
    use = L.rows_of(shape)
    assert len(fit.problems) == len(use) * len(L.LABELS) * len(L.PARITY_CS)
    for p, (t, c, r) in enumerate(fit.problems):
        nt, s = L.NUM_CLASSES[t], rows[use[r]]
        assert status[p] == 0 and iters[p] < 1000, (shape, t, c, r, status[p], iters[p], gn[p])
        W, b = coef[p, :nt], icpt[p, :nt]
        pres = L.present_classes(T[:, t], s, nt)
        assert np.isneginf(b[~pres]).all() and np.isfinite(b[pres]).all() and not W[~pres].any() and not coef[p, nt:].any()
        F, gW, gb = L.value_and_grad(X, T[:, t], s, c, W, np.where(pres, b, 0.0), nt)
        bF, bG = L.value_grad_bound(X, s, c, W, np.where(pres, b, 0.0), nt)
        g = max(np.abs(gW).max(), np.abs(gb).max())
        gap = np.abs(_probs(fit, p, Xq) - ref[(t, use[r], c)]["probs"]).max()
        print(f"N {N} D {D} label {t} C {c} row {use[r]}: {iters[p]} iterations, |grad| {g:.2e} (kernel {gn[p]:.2e}), "
              f"probability gap {gap:.2e} (<= {L.PARITY_BOUND[c]:.2e})")
        assert g <= GTOL + bG, (shape, t, c, r, g)
        assert gap <= L.PARITY_BOUND[c], (shape, t, c, r, gap)
        assert abs(float(fit.objective[p]) - F) <= bF


def test_multiplicity_row_equals_repeated_rows():
    from sm3hip import logreg
    N, D = 17, 33
    X, T, Xq, rows = _case(N, D)
    mult = rows[2].astype(np.int64)
    rep = np.repeat(np.arange(N), mult)
    fit = fitted(N, D)
    big = logreg.fit(torch.from_numpy(X[rep]).to(_dev()), torch.from_numpy(T[rep]), L.PARITY_CS, labels=L.LABELS, gtol=GTOL)
    for t in L.LABELS:
        for c in L.PARITY_CS:
            gap = np.abs(_probs(fit, fit.index(t, c, 2), Xq) - _probs(big, big.index(t, c, 0), Xq)).max()
            print(f"label {t} C {c}: multiplicities against repeated rows {gap:.2e}")
            assert gap <= L.PARITY_BOUND[c]


def test_class_without_weight_and_one_class_problem():
    from sm3hip import logreg
    N, D = 65, 130
    X, T, Xq, rows = _case(N, D)
    fit = fitted(N, D)
    for c in L.PARITY_CS:                                                          # PN under the row that drops its class 1
        p = fit.index(1, c, 3)
        pr = _probs(fit, p, Xq)
        assert not pr[:, 1].any() and not fit.coef[p, 1].any() and float(fit.intercept[p, 1]) == -np.inf
        assert np.abs(pr.sum(axis=1) - 1.0).max() < 1e-12
    one = rows[0].copy()
    one[T[:, 2] == 1] = 0.0                                                        # BWV keeps class 0 alone
    w = torch.from_numpy(np.stack([rows[0], one]))
    base = [(t, c, 0) for t in L.LABELS for c in L.PARITY_CS]
    a = logreg.fit_problems(torch.from_numpy(X).to(_dev()), torch.from_numpy(T), base, weights=w, gtol=GTOL)
    mixed = base[:4] + [(2, 1.0, 1)] + base[4:]
    b = logreg.fit_problems(torch.from_numpy(X).to(_dev()), torch.from_numpy(T), mixed, weights=w, gtol=GTOL)
    assert int(b.status[4]) == 3 and logreg.STATUS[3] == "one_class" and int(b.iterations[4]) == 0
    assert not b.coef[4].any() and b.intercept[4, :2].tolist() == [0.0, -np.inf]
    keep = [i for i in range(len(mixed)) if i != 4]
    for name in ("coef", "intercept", "status", "iterations", "objective", "grad_norm"):
        assert torch.equal(getattr(a, name), getattr(b, name)[keep]), name


# ---- bits ---------------------------------------------------------------------------------------------------------------
def test_a_problem_is_the_same_bits_alone_in_a_batch_and_for_any_chunk():
    from sm3hip import logreg
    N, D = 17, 33
    X, T, Xq, rows = _case(N, D)
    Xd, Tt, w = torch.from_numpy(X).to(_dev()), torch.from_numpy(T), torch.from_numpy(rows)
    batch = [(t, c, r) for r in range(4) for t in L.LABELS for c in L.PARITY_CS] + [(0, 3.0, 1)]
    assert len(batch) == 37
    full = logreg.fit_problems(Xd, Tt, batch, weights=w, gtol=GTOL)
    names = ("coef", "intercept", "status", "iterations", "objective", "grad_norm")
    for pos in (0, 36):
        alone = logreg.fit_problems(Xd, Tt, [batch[pos]], weights=w, gtol=GTOL)
        nt = alone.coef.shape[1]
        for name in names:
            x, y = getattr(alone, name)[0], getattr(full, name)[pos]
            assert torch.equal(x, y[:nt] if name in ("coef", "intercept") else y), (pos, name)
    moved = logreg.fit_problems(Xd, Tt, batch[::-1], weights=w, gtol=GTOL)
    for name in names:
        assert torch.equal(getattr(moved, name).flip(0), getattr(full, name)), name
    # chunk: problems a launch; launch_iters: iterations a launch (the solver state is saved and resumed between launches)
    for kw in (dict(chunk=1), dict(chunk=5), dict(chunk=37), dict(launch_iters=1), dict(launch_iters=7, chunk=5)):
        again = logreg.fit_problems(Xd, Tt, batch, weights=w, gtol=GTOL, **kw)
        for name in names:
            assert torch.equal(getattr(again, name), getattr(full, name)), (kw, name)
    assert int(full.iterations.max()) > 7                                          # so the launches above were cut inside a fit
    Xqd = torch.from_numpy(Xq).to(_dev())
    z = logreg.predict_all(full, Xqd)
    assert torch.equal(z, logreg.predict_all(full, Xqd))
    for i in range(Xq.shape[0]):
        assert torch.equal(logreg.predict_all(full, Xqd[i:i + 1])[:, 0], z[:, i]), i


# ---- sentinels and refusals ---------------------------------------------------------------------------------------------
def test_outputs_stay_inside_their_buffers():
    from exact_inputs import Guarded
    from sm3hip import ops
    N, D, Qn = 17, 33, 5
    X, T, Xq, rows = _case(N, D)
    problems = [(2, 1.0, 0), (0, 0.01, 1), (1, 100.0, 3)]
    P = len(problems)
    dev = _dev()
    Xd, Td = torch.from_numpy(X).to(dev), torch.from_numpy(T).int().to(dev)
    wd = torch.from_numpy(rows).to(dev)
    table = torch.tensor([[t, r, L.NUM_CLASSES[t], 0] for t, _, r in problems], dtype=torch.int32, device=dev)
    Cs = torch.tensor([c for _, c, _ in problems], dtype=torch.float64, device=dev)
    ws = Guarded(P * ops.logreg_workspace(N, D, True), torch.float64)
    coef, icpt = Guarded(P * 8 * D, torch.float64), Guarded(P * 8, torch.float64)
    info, res = Guarded(P * 2, torch.int32), Guarded(P * 2, torch.float64)
    ops.logreg_fit(Xd, Td, wd, table, Cs, GTOL, 1000, ws.t, coef.t.view(P, 8, D), icpt.t.view(P, 8), info.t.view(P, 2), res.t.view(P, 2),
                   iters=3)
    torch.cuda.synchronize()
    assert all(g.guards() for g in (ws, coef, icpt, info, res))
    assert info.t.view(P, 2).tolist() == [[ops.LOGREG_RUNNING, 3]] * 3            # one launch of 3 iterations: none has finished
    while bool((info.t.view(P, 2)[:, 0] == ops.LOGREG_RUNNING).any()):
        ops.logreg_fit(Xd, Td, wd, table, Cs, GTOL, 1000, ws.t, coef.t.view(P, 8, D), icpt.t.view(P, 8), info.t.view(P, 2),
                       res.t.view(P, 2), resume=True, iters=3)
    torch.cuda.synchronize()
    assert all(g.guards() for g in (ws, coef, icpt, info, res))
    assert info.t.view(P, 2)[:, 0].tolist() == [0, 0, 0] and bool(torch.isfinite(coef.t).all())
    ws2 = Guarded(P * ops.logreg_workspace(N, D, False), torch.float64)
    F, gW, gb = Guarded(P, torch.float64), Guarded(P * 8 * D, torch.float64), Guarded(P * 8, torch.float64)
    b0 = torch.where(torch.isfinite(icpt.t), icpt.t, torch.zeros_like(icpt.t)).view(P, 8).contiguous()
    ops.logreg_value_grad(Xd, Td, wd, table, Cs, coef.t.view(P, 8, D).clone(), b0, ws2.t, F.t, gW.t.view(P, 8, D), gb.t.view(P, 8))
    torch.cuda.synchronize()
    assert all(g.guards() for g in (ws2, F, gW, gb)) and float(gW.t.abs().max()) <= GTOL * 1.01
    logits = Guarded(P * Qn * 8, torch.float64)
    nts = torch.tensor([L.NUM_CLASSES[t] for t, _, _ in problems], dtype=torch.int32, device=dev)
    ops.logreg_predict(torch.from_numpy(Xq[:Qn]).to(dev), coef.t.view(P, 8, D), icpt.t.view(P, 8), nts, logits.t.view(P, Qn, 8))
    torch.cuda.synchronize()
    assert logits.guards() and not logits.t.view(P, Qn, 8)[0, :, 2:].any()


def test_refusals_raise_on_the_host():
    """Every refusal is a ValueError of the host-side checks; that no kernel is launched behind them is what
    tests/test_logreg_cpu.py shows, where the same checks run with no device at all."""
    from sm3hip import logreg, ops
    N, D = 17, 33
    X, T, _, rows = _case(N, D)
    Xd, Tt, w = torch.from_numpy(X).to(_dev()), torch.from_numpy(T), torch.from_numpy(rows)
    bad_t = Tt.clone()
    bad_t[3, 0] = 5
    neg, nan = w.clone(), w.clone()
    neg[1, 2], nan[0, 0] = -1.0, float("nan")
    for kw in (dict(targets=bad_t), dict(weights=neg), dict(weights=nan), dict(Cs=[1.0, -1.0]), dict(Cs=[float("inf")]),
               dict(Cs=[float("nan")])):
        args = {**dict(targets=Tt, Cs=[1.0], weights=w, labels=L.LABELS), **kw}
        with pytest.raises(ValueError, match="logreg"):
            logreg.fit(Xd, **args)
    with pytest.raises(ValueError, match="problem"):
        logreg.fit_problems(Xd, Tt, [(0, 1.0, 4)], weights=w)                    # a weight row that is not there
    with pytest.raises(ValueError, match="MAX_DIM"):
        logreg.fit(torch.zeros(4, logreg.MAX_DIM + 1), torch.zeros(4, 8, dtype=torch.long))
    with pytest.raises(ValueError, match="MAX_ROWS"):
        logreg.fit(torch.zeros(logreg.MAX_ROWS + 1, 1), torch.zeros(logreg.MAX_ROWS + 1, 8, dtype=torch.long))
    with pytest.raises(ValueError, match="GPU"):
        logreg.fit(Xd.cpu(), Tt, [1.0])
    f = fitted(N, D)
    with pytest.raises(ValueError, match="features"):
        logreg.predict_all(f, torch.zeros(2, D + 1, device=_dev()))
    with pytest.raises(ValueError, match="workspace"):
        ops.logreg_fit(Xd, Tt.int().to(_dev()), w.to(_dev()), torch.tensor([[0, 0, 5, 0]], dtype=torch.int32, device=_dev()),
                       torch.ones(1, dtype=torch.float64, device=_dev()), GTOL, 10, torch.empty(8, dtype=torch.float64, device=_dev()),
                       torch.empty(1, 8, D, dtype=torch.float64, device=_dev()), torch.empty(1, 8, dtype=torch.float64, device=_dev()),
                       torch.empty(1, 2, dtype=torch.int32, device=_dev()), torch.empty(1, 2, dtype=torch.float64, device=_dev()))


# ---- host-side pieces on the device's results ---------------------------------------------------------------------------
def test_select_and_baseline_heads_on_a_fit():
    from sm3hip import logreg
    from src.models.baseline import NUM_CLASSES
    rs = np.random.RandomState(3)
    N, D = 96, 40
    X = torch.from_numpy((rs.randn(N, D) * 3.0 + 1.5).astype(np.float32)).to(_dev())
    T = torch.from_numpy(np.stack([rs.randint(0, n, N) for n in NUM_CLASSES], axis=1))
    norm = logreg.normalize_fit(X, "standardize")
    Xn = logreg.normalize_apply(X, norm)
    cv = logreg.fit(Xn, T, [0.01, 1.0], weights=logreg.folds(N, 3, 0), gtol=GTOL)
    sel = logreg.select(cv, by="nll", X=Xn, targets=T)
    assert len(sel["C"]) == 8 and set(sel["C"]) <= {0.01, 1.0} and tuple(sel["table"].shape) == (8, 2)
    grid = logreg.fit(Xn[:64], T[:64], [0.01, 1.0], gtol=GTOL)                    # the validation path: rows 64 .. 95 held out
    for by in ("auc", "nll"):
        val = logreg.select(grid, Xn[64:].contiguous(), T[64:], by=by)
        zv = logreg.predict_all(grid, Xn[64:].contiguous())
        for t in range(8):
            want = [logreg.score(zv[grid.index(t, c), :, :NUM_CLASSES[t]], T[64:, t].to(_dev()), t, by) for c in (0.01, 1.0)]
            assert val["table"][t].tolist() == want and val["C"][t] == (1.0 if want[1] > want[0] else 0.01)
        shared = logreg.select(grid, Xn[64:].contiguous(), T[64:], by=by, per_label=False)
        assert len(set(shared["C"])) == 1 and torch.equal(shared["table"], val["table"])
    fit = logreg.fit(Xn, T, [1.0], gtol=GTOL)
    which = [fit.index(t, 1.0) for t in range(8)]
    z = logreg.predict_logits(fit, Xn, which)
    state = logreg.to_baseline_state(fit, which, norm)
    for t in range(8):
        head = torch.nn.Linear(D, NUM_CLASSES[t])
        head.load_state_dict({"weight": state[f"classifier.{t}.weight"], "bias": state[f"classifier.{t}.bias"]})
        got = head.to(_dev())(X).double().detach()
        # fp32 rounding of a D-term dot product of magnitudes |w| |x|, and of the folded map (x - mean) / std itself
        tol = 4 * (D + 2) * 2.0 ** -24 * float((state[f"classifier.{t}.weight"].abs().double().to(_dev()) @ X.abs().double().T).max() + 1)
        assert float((got - z[t]).abs().max()) <= tol, (t, float((got - z[t]).abs().max()), tol)
    with pytest.raises(ValueError, match="l2"):
        logreg.to_baseline_state(fit, which, logreg.normalize_fit(X, "l2"))


# ---- the tool -----------------------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("sm3_logreg_cli", os.path.join(TOOLS, "backbone_logreg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_end_to_end_on_random_features(tmp_path):
    from sm3hip import report
    from src.models.baseline import NUM_CLASSES
    tool = _tool()
    outs = []
    for run in ("a", "b"):
        log = tmp_path / run
        stat = tool.main(["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "--log-path", str(log),
                          "--random-features", "96", "40", "64", "--logreg-c", "0.01", "1", "100", "--save-features"])
        assert stat["problems"] == 24 and stat["not_converged"] == 0 and 0.0 <= stat["AUC_AVG"] <= 1.0
        outs.append(torch.load(log / "logreg_predictions.pt", weights_only=False))
        for f in ("best_linear.pth", "val_report.json", "val_report.csv", "logreg_curve.csv"):
            assert (log / f).is_file(), f
    a, b = outs
    preds, targets = report.load_predictions(str(tmp_path / "a" / "logreg_predictions.pt"))
    assert len(preds) == 8 and tuple(targets.shape) == (40, 8) and [p.shape[1] for p in preds] == NUM_CLASSES
    for x, y in zip(a["preds"], b["preds"]):
        assert torch.equal(x, y)
    assert a["C"] == b["C"] and torch.equal(a["selection"]["val_auc"], b["selection"]["val_auc"])
    assert torch.equal(a["status"][0]["grad_norm"], b["status"][0]["grad_norm"])
    sa = torch.load(tmp_path / "a" / "best_linear.pth", weights_only=False)["state_dict"]
    sb = torch.load(tmp_path / "b" / "best_linear.pth", weights_only=False)["state_dict"]
    assert sorted(sa) == sorted(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert len(open(tmp_path / "a" / "logreg_curve.csv").read().splitlines()) == 1 + 8 * 3
    # the default run (--logreg-normalize standardize, folded into the heads): best_linear.pth on the saved features gives the
    # saved logits to fp32 rounding -- of a 64-term dot product of magnitudes |w| |x|, of the weights and of the features' scaling
    x, seen = a["test_features"], 0.0
    assert a["normalize"] == "standardize" and tuple(x.shape) == (40, 64) and tuple(a["train_features"].shape) == (96, 64)
    for t in range(8):
        w, bias = sa[f"classifier.{t}.weight"], sa[f"classifier.{t}.bias"]
        got = torch.nn.functional.linear(x, w, bias).double()
        tol = 4 * (64 + 2) * 2.0 ** -24 * float((w.abs().double() @ x.abs().double().T).max() + 1)
        err = float((got - a["preds"][t]).abs().max())
        print(f"label {t}: heads on the saved features against the saved logits {err:.2e} (<= {tol:.2e})")
        assert err <= tol, (t, err, tol)
        unfolded = torch.nn.functional.linear(x, w * a["train_features"].double().std(dim=0, unbiased=False).float(), bias).double()
        seen = max(seen, float((unfolded - a["preds"][t]).abs().max()) / tol)
    assert seen > 10                                                              # the check would see heads without the fold


def test_tool_through_the_resnet18_encoders(tmp_path):
    tool = _tool()
    stat = tool.main(["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "--log-path", str(tmp_path), "-b", "4",
                      "--img-sz", "64", "64", "--steps-per-epoch", "6", "--val-steps", "3", "--logreg-c", "0.01", "1",
                      "--logreg-select", "cv", "--logreg-folds", "3"])
    assert stat["problems"] >= 16 + 3 * 16 and stat["pairs_per_s"] > 0
    d = torch.load(tmp_path / "logreg_predictions.pt", weights_only=False)
    assert tuple(d["targets"].shape) == (12, 8) and tuple(d["preds"][0].shape) == (12, 5)
    state = torch.load(tmp_path / "best_linear.pth", weights_only=False)["state_dict"]
    from src.models.baseline import Baseline
    model = Baseline("resnet18", None)
    model.load_state_dict(state)
    assert tuple(model.classifier[0].weight.shape) == (5, 1024)


def test_tool_fractions_balanced_l2_and_the_optional_reports(tmp_path):
    tool = _tool()
    stat = tool.main(["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "--log-path", str(tmp_path),
                      "--random-features", "96", "40", "64", "--logreg-c", "0.1", "10", "--logreg-fractions", "0.25", "1", "0.5",
                      "--logreg-class-weight", "balanced", "--logreg-normalize", "l2", "--logreg-by", "nll", "--logreg-shared-c",
                      "--logreg-refit-trainval", "--calibration", "--operating", "--checklist"])
    assert stat["problems"] == 3 * 8 * 2 + 8 and len(set(stat["C"])) == 1 and stat["not_converged"] == 0
    assert not (tmp_path / "best_linear.pth").exists()                              # l2: no heads can hold it
    for f in ("logreg_predictions.pt", "val_report.json", "val_calibration.json", "val_operating.json", "val_checklist.json"):
        assert (tmp_path / f).is_file(), f
    lines = open(tmp_path / "logreg_curve.csv").read().splitlines()
    assert lines[0] == "label,C,fraction,val_auc,val_nll" and len(lines) == 1 + 3 * 8 * 2
    assert {ln.split(",")[2] for ln in lines[1:]} == {"1.0", "0.5", "0.25"}
    d = torch.load(tmp_path / "logreg_predictions.pt", weights_only=False)
    assert d["selection"]["fractions"] == [1.0, 0.5, 0.25] and tuple(d["selection"]["val_nll"].shape) == (3, 8, 2)


def test_explanations_run_on_heads_of_a_fit_that_lacked_a_class():
    """A class without weight gets coefficient row 0 and bias -inf in best_linear.pth.  Grad-CAM, Integrated Gradients, RISE and the
    deletion / insertion curves on a Baseline with such heads: every output finite, the class never predicted."""
    from sm3hip import logreg
    from sm3hip.attr import integrated_gradients
    from sm3hip.cam import grad_cam
    from sm3hip.faith import deletion_insertion
    from sm3hip.rise import rise
    from src.models.baseline import Baseline, NUM_CLASSES
    rs = np.random.RandomState(11)
    N, D = 48, 1024                                                                # the width of the ResNet-18 pair
    X = torch.from_numpy(rs.randn(N, D).astype(np.float32)).to(_dev())
    T = np.stack([rs.randint(0, n, N) for n in NUM_CLASSES], axis=1)
    w = np.ones(N)
    w[T[:, 1] == 1] = 0.0                                                          # PN loses its class 1
    fit = logreg.fit(X, torch.from_numpy(T), [1.0], weights=torch.from_numpy(w), gtol=GTOL)
    which = [fit.index(t, 1.0) for t in range(8)]
    state = logreg.to_baseline_state(fit, which, logreg.normalize_fit(X, "none"))
    assert state["classifier.1.bias"].tolist()[1] == -np.inf and not state["classifier.1.weight"][1].any()
    torch.manual_seed(0)
    model = Baseline("resnet18", None)
    assert not model.load_state_dict(state, strict=False).unexpected_keys
    for b in (model.derm_backbone, model.clinic_backbone):
        b.sm3_dtype = torch.float32
    model = model.to(_dev()).eval()
    derm, clinic = torch.randn(2, 3, 64, 64, device=_dev()), torch.randn(2, 3, 64, 64, device=_dev())
    cam = grad_cam(model, derm, clinic, layer="layer4", target="pred")
    ig = integrated_gradients(model, derm, clinic, target="pred", steps=4)
    rz = rise(model, derm, clinic, target="pred", masks=16, cells=7, p=0.5, seed=0)
    for name, out in (("cam", cam), ("ig", ig), ("rise", rz)):
        assert bool(torch.isfinite(out["maps"]).all()), name
        assert not bool((out["target_class"][:, 1] == 1).any()), name              # the class of logit -inf is never the argmax
    curves = deletion_insertion(model, derm, clinic, cam["maps"], target="pred", steps=4)
    for k, v in curves.items():
        if isinstance(v, torch.Tensor) and v.is_floating_point():
            assert bool(torch.isfinite(v).all()), k
