"""GPU: the lockstep solver of the logistic-regression probe (csrc/logreg.hip, sm3hip/logreg.py solver="lockstep")
-- the two batched f64-MFMA products on their own, value_and_grad and fit through them, the bits contract, the tool.

  * products, integer inputs (X in [-3, 3], V integers / 16, vb integers / 4, R integers / 8: every sum is exact in any order) ==
    numpy, at N, D on either side of multiples of 4 and 16, across a slab boundary of the gradient's rows, 1 to 37 problems of 2,
    3 and 5 classes; an inactive problem and every entry outside the listed columns keeps its sentinel; guard bands stay;
  * products, random inputs: a problem alone == the same problem at each place of a batch of 37 and of the reversed batch;
  * value_and_grad(solver="lockstep") within logreg_inputs.value_grad_bound of the numpy restatement (the bound is for sums that
    differ in ORDER only, which is all that differs), on random and on integer inputs;
  * fit(solver="lockstep") on every shape of logreg_inputs.SHAPES: status ok, the restatement's |grad F|_inf at the returned point
    <= gtol + bound, probabilities within PARITY_BOUND[C] of the restatement's optimum, within 2 PARITY_BOUND[C] of the workgroup
    solver's (both lie within the bound of the same optimum);
  * bits: alone == in a batch of 37, reversed, chunk 1 / 5 / 37, launch_iters 1 / 7, twice; a one-class problem in the middle;
    max_iter = 3; a fit that ends without a step (gtol = 0) returns its last point, as the workgroup solver does;
  * refusals on the host, sentinel-padded outputs, the tool end to end with --logreg-solver lockstep."""
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
SENTINEL = -777.25
NAMES = ("coef", "intercept", "status", "iterations", "objective", "grad_norm")


def _dev():
    return torch.device("cuda", 0)


def _case(N, D):
    X, T, Xq = L.make_case(N, D)
    return X, T, Xq, L.case_rows(N, T)


def _slab():
    from sm3hip import ops
    return ops.LOGREG_LOCKSTEP_SLAB


def _product_shapes():
    s = 2048  # ops.LOGREG_LOCKSTEP_SLAB, asserted below: the parametrisation runs before the library is loaded
    return ((1, 1), (3, 5), (17, 33), (65, 130), (130, 515), (17, 1030), (s + 1, 33), (2 * s + 3, 5))


# ---- the products -----------------------------------------------------------------------------------------------------------
def _run_products(X, V, vb, Rm, nts, active):
    """(Z [P, N, 8], G [P, 8, D], gb [P, 8]) numpy from sentinel-filled, guarded buffers."""
    from exact_inputs import Guarded
    from sm3hip import ops
    dev = _dev()
    (N, D), P = X.shape, len(nts)
    cols = ops.logreg_columns(nts).to(dev)
    act = torch.tensor(active, dtype=torch.int32, device=dev)
    Xd = torch.from_numpy(X).to(dev)
    Z, G, gb = Guarded(P * N * 8, torch.float64), Guarded(P * 8 * D, torch.float64), Guarded(P * 8, torch.float64)
    ws = Guarded(-(-N // ops.LOGREG_LOCKSTEP_SLAB) * cols.numel() * D, torch.float64)
    for g in (Z, G, gb):
        g.t.fill_(SENTINEL)
    ops.logreg_batch_logits(Xd, torch.from_numpy(V).to(dev), None if vb is None else torch.from_numpy(vb).to(dev), cols, act,
                            Z.t.view(P, N, 8))
    ops.logreg_batch_grad(Xd, torch.from_numpy(Rm).to(dev), cols, act, ws.t, G.t.view(P, 8, D), gb.t.view(P, 8))
    torch.cuda.synchronize()
    assert all(g.guards() for g in (Z, G, gb, ws))
    return Z.t.view(P, N, 8).cpu().numpy(), G.t.view(P, 8, D).cpu().numpy(), gb.t.view(P, 8).cpu().numpy()


@pytest.mark.parametrize("P", (1, 2, 3, 37))
@pytest.mark.parametrize("shape", _product_shapes())
def test_products_on_integer_inputs_equal_numpy(shape, P):
    N, D = shape
    assert _slab() == 2048
    rs = np.random.RandomState(100 * P + N + D)
    X = rs.randint(-3, 4, (N, D)).astype(np.float32)
    V, vb = rs.randint(-8, 9, (P, 8, D)) / 16.0, rs.randint(-8, 9, (P, 8)) / 4.0
    Rm = rs.randint(-8, 9, (P, N, 8)) / 8.0
    nts = [(2, 3, 5)[(p + P) % 3] for p in range(P)]
    X64 = X.astype(np.float64)
    for active in ([1] * P, [p % 2 for p in range(P)], [0] * P):
        Z, G, gb = _run_products(X, V, vb, Rm, nts, active)
        for p, nt in enumerate(nts):
            live = nt if active[p] else 0
            assert np.array_equal(Z[p, :, :live], X64 @ V[p, :live].T + vb[p, :live]), (shape, P, p, "logits")
            assert np.array_equal(G[p, :live], Rm[p, :, :live].T @ X64), (shape, P, p, "gradient")
            assert np.array_equal(gb[p, :live], Rm[p, :, :live].sum(axis=0)), (shape, P, p, "gb")
            assert (Z[p, :, live:] == SENTINEL).all() and (G[p, live:] == SENTINEL).all() and (gb[p, live:] == SENTINEL).all(), \
                (shape, P, p, "an entry outside the live columns was written")
    Z0 = _run_products(X, V, None, Rm, nts, [1] * P)[0]                             # no intercepts: the sum alone
    for p, nt in enumerate(nts):
        assert np.array_equal(Z0[p, :, :nt], X64 @ V[p, :nt].T)


def test_products_a_problem_alone_equals_it_anywhere_in_a_batch():
    N, D, P = 65, 130, 37
    rs = np.random.RandomState(9)
    X = rs.randn(N, D).astype(np.float32)
    V, vb, Rm = rs.randn(P, 8, D), rs.randn(P, 8), rs.randn(P, N, 8)
    nts = [(5, 3, 2)[p % 3] for p in range(P)]
    Z, G, gb = _run_products(X, V, vb, Rm, nts, [1] * P)
    Zr, Gr, gbr = _run_products(X, V[::-1].copy(), vb[::-1].copy(), Rm[::-1].copy(), nts[::-1], [1] * P)
    half = [p % 2 for p in range(P)]                                                # the neighbours switched off
    Zh, Gh, gbh = _run_products(X, V, vb, Rm, nts, half)
    for p, nt in enumerate(nts):
        Za, Ga, gba = _run_products(X, V[p:p + 1], vb[p:p + 1], Rm[p:p + 1], nts[p:p + 1], [1])
        for name, alone, batch, moved, masked in (("logits", Za[0, :, :nt], Z[p, :, :nt], Zr[P - 1 - p, :, :nt], Zh[p, :, :nt]),
                                                  ("gradient", Ga[0, :nt], G[p, :nt], Gr[P - 1 - p, :nt], Gh[p, :nt]),
                                                  ("gb", gba[0, :nt], gb[p, :nt], gbr[P - 1 - p, :nt], gbh[p, :nt])):
            assert np.array_equal(alone, batch) and np.array_equal(alone, moved), (p, name)
            assert not half[p] or np.array_equal(alone, masked), (p, name)


# ---- value and gradient -------------------------------------------------------------------------------------------------------
def _check_value_grad(X, T, rows, W, b, Cs, tag):
    from sm3hip import logreg
    problems = [(t, Cs[(t + r) % len(Cs)], r) for t in L.LABELS for r in range(rows.shape[0])]
    P, D = len(problems), X.shape[1]
    Wp, bp = np.zeros((P, 5, D)), np.zeros((P, 5))
    for p, (t, _, _) in enumerate(problems):
        nt = L.NUM_CLASSES[t]
        Wp[p, :nt], bp[p, :nt] = W[p % len(W), :nt], b[p % len(b), :nt]
    F, gW, gb = logreg.value_and_grad(torch.from_numpy(X).to(_dev()), torch.from_numpy(T), problems, torch.from_numpy(Wp),
                                      torch.from_numpy(bp), weights=torch.from_numpy(rows), solver="lockstep")
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


# ---- the fit ------------------------------------------------------------------------------------------------------------------
def _probs(fit, p, Xq):
    from sm3hip import logreg
    nt = fit.n_classes[p]
    z = logreg.predict_all(fit, torch.from_numpy(Xq).to(_dev()), [p])[0, :, :nt]
    return torch.softmax(z, dim=1).cpu().numpy()


@pytest.mark.parametrize("shape", L.SHAPES)
def test_fit_certificate_optimum_and_the_workgroup_solver(shape):
    from sm3hip import logreg
    N, D = shape
    X, T, Xq, rows = _case(N, D)
    use, ref = L.rows_of(shape), L.reference(N, D)
    args = (torch.from_numpy(X).to(_dev()), torch.from_numpy(T), L.PARITY_CS)
    kw = dict(weights=torch.from_numpy(rows[list(use)]), labels=L.LABELS, gtol=GTOL)
    fit, other = logreg.fit(*args, solver="lockstep", **kw), logreg.fit(*args, solver="workgroup", **kw)
    assert fit.solver == "lockstep" and other.solver == "workgroup" and fit.problems == other.problems
    status, iters = fit.status.cpu().numpy(), fit.iterations.cpu().numpy()
    coef, icpt, gn = fit.coef.cpu().numpy(), fit.intercept.cpu().numpy(), fit.grad_norm.cpu().numpy()
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
        mine = _probs(fit, p, Xq)
        gap, between = np.abs(mine - ref[(t, use[r], c)]["probs"]).max(), np.abs(mine - _probs(other, p, Xq)).max()
        print(f"N {N} D {D} label {t} C {c} row {use[r]}: {iters[p]} iterations (workgroup {int(other.iterations[p])}), |grad| {g:.2e} "
              f"(kernel {gn[p]:.2e}), probability gap {gap:.2e} (<= {L.PARITY_BOUND[c]:.2e}), to the workgroup solver {between:.2e}")
        assert g <= GTOL + bG, (shape, t, c, r, g)
        assert gap <= L.PARITY_BOUND[c], (shape, t, c, r, gap)
        assert between <= 2.0 * L.PARITY_BOUND[c], (shape, t, c, r, between)
        assert abs(float(fit.objective[p]) - F) <= bF


# ---- bits ---------------------------------------------------------------------------------------------------------------------
def _batch37():
    N, D = 17, 33
    X, T, _, rows = _case(N, D)
    batch = [(t, c, r) for r in range(4) for t in L.LABELS for c in L.PARITY_CS] + [(0, 3.0, 1)]
    assert len(batch) == 37
    return torch.from_numpy(X).to(_dev()), torch.from_numpy(T), torch.from_numpy(rows), batch


def _same(a, b, pa, pb, what):
    nt = min(a.coef.shape[1], b.coef.shape[1])
    for name in NAMES:
        x, y = getattr(a, name)[pa], getattr(b, name)[pb]
        if name in ("coef", "intercept"):
            assert not x[nt:].any() and not y[nt:].any()
            x, y = x[:nt], y[:nt]
        assert torch.equal(x, y), (what, name)


def test_a_problem_is_the_same_bits_alone_in_a_batch_for_any_chunk_and_any_cut():
    from sm3hip import logreg
    Xd, Tt, w, batch = _batch37()
    kw = dict(weights=w, gtol=GTOL, solver="lockstep")
    full = logreg.fit_problems(Xd, Tt, batch, **kw)
    assert bool((full.status == 0).all()) and int(full.iterations.max()) > 7      # so launch_iters=7 cuts inside a fit
    for pos in (0, 36):
        _same(logreg.fit_problems(Xd, Tt, [batch[pos]], **kw), full, 0, pos, ("alone", pos))
    moved = logreg.fit_problems(Xd, Tt, batch[::-1], **kw)
    for name in NAMES:
        assert torch.equal(getattr(moved, name).flip(0), getattr(full, name)), ("reversed", name)
    for extra in (dict(chunk=1), dict(chunk=5), dict(chunk=37), dict(launch_iters=1), dict(launch_iters=7), dict()):
        again = logreg.fit_problems(Xd, Tt, batch, **kw, **extra)
        for name in NAMES:
            assert torch.equal(getattr(again, name), getattr(full, name)), (extra, name)


def test_a_one_class_problem_in_the_middle_changes_nothing_else():
    from sm3hip import logreg
    N, D = 65, 130
    X, T, _, rows = _case(N, D)
    one = rows[0].copy()
    one[T[:, 2] == 1] = 0.0                                                        # BWV keeps class 0 alone
    w = torch.from_numpy(np.stack([rows[0], one]))
    Xd, Tt = torch.from_numpy(X).to(_dev()), torch.from_numpy(T)
    base = [(t, c, 0) for t in L.LABELS for c in L.PARITY_CS]
    a = logreg.fit_problems(Xd, Tt, base, weights=w, gtol=GTOL, solver="lockstep")
    mixed = base[:4] + [(2, 1.0, 1)] + base[4:]
    b = logreg.fit_problems(Xd, Tt, mixed, weights=w, gtol=GTOL, solver="lockstep")
    assert int(b.status[4]) == 3 and int(b.iterations[4]) == 0
    assert not b.coef[4].any() and b.intercept[4, :2].tolist() == [0.0, -np.inf]
    keep = [i for i in range(len(mixed)) if i != 4]
    for name in NAMES:
        assert torch.equal(getattr(a, name), getattr(b, name)[keep]), name


def test_max_iter_three_stops_after_three_iterations_alone_as_in_the_batch():
    from sm3hip import logreg
    Xd, Tt, w, batch = _batch37()
    kw = dict(weights=w, gtol=GTOL, solver="lockstep")
    need = logreg.fit_problems(Xd, Tt, batch, **kw).iterations
    short = logreg.fit_problems(Xd, Tt, batch, max_iter=3, **kw)
    more = need > 3
    assert bool(more.any())
    assert bool((short.status[more] == 1).all()) and bool((short.iterations[more] == 3).all())
    assert bool((short.status[~more] == 0).all()) and torch.equal(short.iterations[~more], need[~more])
    for pos in (0, 17, 36):
        _same(logreg.fit_problems(Xd, Tt, [batch[pos]], max_iter=3, **kw), short, 0, pos, ("max_iter", pos))
    cut = logreg.fit_problems(Xd, Tt, batch, max_iter=3, launch_iters=2, chunk=5, **kw)
    for name in NAMES:
        assert torch.equal(getattr(cut, name), getattr(short, name)), name


def test_a_fit_that_ends_without_a_step_returns_its_last_point():
    """gtol = 0 cannot be met: a problem goes on until its line search finds no step (status 2) or max_iter is reached (status 1).
    Either way the returned coef / intercept are the last point -- the one `objective` and `grad_norm` speak of -- as the
    workgroup solver returns it, and the bits contract holds."""
    from sm3hip import logreg
    N, D = 17, 33
    X, T, Xq, rows = _case(N, D)
    Xd, Tt, w, batch = _batch37()
    kw = dict(weights=w, gtol=0.0, max_iter=300)
    full, other = logreg.fit_problems(Xd, Tt, batch, solver="lockstep", **kw), logreg.fit_problems(Xd, Tt, batch, solver="workgroup", **kw)
    status, coef, icpt = full.status.cpu().numpy(), full.coef.cpu().numpy(), full.intercept.cpu().numpy()
    print("statuses", status.tolist(), "iterations", full.iterations.tolist())
    assert set(status.tolist()) <= {1, 2} and (status == 2).any()
    for p, (t, c, r) in enumerate(batch):
        nt, s = L.NUM_CLASSES[t], rows[r]
        pres = L.present_classes(T[:, t], s, nt)
        W, b = coef[p, :nt], icpt[p, :nt]
        assert W[pres].any() and not W[~pres].any() and np.isneginf(b[~pres]).all() and np.isfinite(b[pres]).all(), (p, status[p])
        F, gW, gb = L.value_and_grad(X, T[:, t], s, c, W, np.where(pres, b, 0.0), nt)
        bF, bG = L.value_grad_bound(X, s, c, W, np.where(pres, b, 0.0), nt)
        g = max(np.abs(gW).max(), np.abs(gb).max())
        bound = L.PARITY_BOUND.get(c, L.PARITY_BOUND[100.0])                       # C = 3 is better conditioned than C = 100
        between = np.abs(_probs(full, p, Xq) - _probs(other, p, Xq)).max()
        print(f"label {t} C {c} row {r}: status {status[p]}, |F - objective| {abs(float(full.objective[p]) - F):.2e} (<= {bF:.2e}), "
              f"|grad| {g:.2e} (kernel {float(full.grad_norm[p]):.2e}), to the workgroup solver {between:.2e} (<= {2 * bound:.2e})")
        assert abs(float(full.objective[p]) - F) <= bF, (p, status[p])
        assert between <= 2.0 * bound, (p, status[p], between)
    for pos in (0, 36, int(np.flatnonzero(status == 2)[0])):
        _same(logreg.fit_problems(Xd, Tt, [batch[pos]], solver="lockstep", **kw), full, 0, pos, ("no step", pos))


# ---- sentinels and refusals ---------------------------------------------------------------------------------------------------
def test_outputs_stay_inside_their_buffers():
    from exact_inputs import Guarded
    from sm3hip import ops
    N, D = 17, 33
    X, T, _, rows = _case(N, D)
    problems = [(2, 1.0, 0), (0, 0.01, 1), (1, 100.0, 3)]
    P = len(problems)
    dev = _dev()
    Xd, Td, wd = torch.from_numpy(X).to(dev), torch.from_numpy(T).int().to(dev), torch.from_numpy(rows).to(dev)
    table = torch.tensor([[t, r, L.NUM_CLASSES[t], 0] for t, _, r in problems], dtype=torch.int32, device=dev)
    Cs = torch.tensor([c for _, c, _ in problems], dtype=torch.float64, device=dev)
    cols = ops.logreg_columns([L.NUM_CLASSES[t] for t, _, _ in problems]).to(dev)
    ws = Guarded(ops.logreg_lockstep_workspace(N, D, P, cols.numel(), True), torch.float64)
    coef, icpt = Guarded(P * 8 * D, torch.float64), Guarded(P * 8, torch.float64)
    info, res = Guarded(P * 2, torch.int32), Guarded(P * 2, torch.float64)
    out = (coef.t.view(P, 8, D), icpt.t.view(P, 8), info.t.view(P, 2), res.t.view(P, 2))
    ops.logreg_fit_lockstep(Xd, Td, wd, table, Cs, cols, GTOL, 1000, ws.t, *out, iters=3)
    torch.cuda.synchronize()
    assert all(g.guards() for g in (ws, coef, icpt, info, res))
    # a call of 3 rounds: the first forms the gradient at zero, two steps follow; the second step's gradient is taken in, and the
    # iteration counted, by the next call's direction kernel
    assert info.t.view(P, 2).tolist() == [[ops.LOGREG_RUNNING, 1]] * 3
    for _ in range(400):
        if not bool((info.t.view(P, 2)[:, 0] == ops.LOGREG_RUNNING).any()):
            break
        ops.logreg_fit_lockstep(Xd, Td, wd, table, Cs, cols, GTOL, 1000, ws.t, *out, resume=True, iters=3)
    torch.cuda.synchronize()
    assert all(g.guards() for g in (ws, coef, icpt, info, res))
    assert info.t.view(P, 2)[:, 0].tolist() == [0, 0, 0] and bool(torch.isfinite(coef.t).all())
    ws2 = Guarded(ops.logreg_lockstep_workspace(N, D, P, cols.numel(), False), torch.float64)
    F, gW, gb = Guarded(P, torch.float64), Guarded(P * 8 * D, torch.float64), Guarded(P * 8, torch.float64)
    b0 = torch.where(torch.isfinite(icpt.t), icpt.t, torch.zeros_like(icpt.t)).view(P, 8).contiguous()
    ops.logreg_value_grad_lockstep(Xd, Td, wd, table, Cs, cols, coef.t.view(P, 8, D).clone(), b0, ws2.t, F.t, gW.t.view(P, 8, D),
                                   gb.t.view(P, 8))
    torch.cuda.synchronize()
    assert all(g.guards() for g in (ws2, F, gW, gb)) and float(gW.t.abs().max()) <= GTOL * 1.01


def test_refusals_raise_on_the_host():
    from sm3hip import logreg, ops
    N, D = 17, 33
    X, T, _, rows = _case(N, D)
    dev = _dev()
    Xd, Tt, w = torch.from_numpy(X).to(dev), torch.from_numpy(T), torch.from_numpy(rows)
    bad_t = Tt.clone()
    bad_t[3, 0] = 5
    neg = w.clone()
    neg[1, 2] = -1.0
    for kw in (dict(targets=bad_t), dict(weights=neg), dict(Cs=[1.0, -1.0]), dict(Cs=[float("nan")])):
        args = {**dict(targets=Tt, Cs=[1.0], weights=w, labels=L.LABELS, solver="lockstep"), **kw}
        with pytest.raises(ValueError, match="logreg"):
            logreg.fit(Xd, **args)
    with pytest.raises(ValueError, match="solver"):
        logreg.fit(Xd, Tt, [1.0], solver="newton")
    with pytest.raises(ValueError, match="solver"):
        logreg.value_and_grad(Xd, Tt, [(0, 1.0, 0)], torch.zeros(1, 5, D), torch.zeros(1, 5), solver="newton")
    with pytest.raises(ValueError, match="GPU"):
        logreg.fit(Xd.cpu(), Tt, [1.0], solver="lockstep")
    with pytest.raises(ValueError, match="chunk"):
        logreg.fit(Xd, Tt, [1.0], solver="lockstep", chunk=0)
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    table, Cs, cols = torch.tensor([[0, 0, 5, 0]], dtype=torch.int32, device=dev), torch.ones(1, dtype=torch.float64, device=dev), \
        ops.logreg_columns([5]).to(dev)
    fit = lambda ws=None, cols=cols, iters=1: ops.logreg_fit_lockstep(
        Xd, Tt.int().to(dev), w.to(dev), table, Cs, cols, GTOL, 10, f64(ops.logreg_lockstep_workspace(N, D, 1, 5)) if ws is None else ws,
        f64(1, 8, D), f64(1, 8), i32(1, 2), f64(1, 2), iters=iters)
    with pytest.raises(ValueError, match="workspace"):
        fit(ws=f64(8))
    with pytest.raises(ValueError, match="columns"):
        fit(cols=i32(9))
    with pytest.raises(ValueError, match="iters"):
        fit(iters=0)
    with pytest.raises(ValueError, match="iters"):
        fit(iters=ops.LOGREG_LOCKSTEP_MAX_ITERS + 1)
    with pytest.raises(ValueError, match="workspace"):
        ops.logreg_batch_grad(Xd, f64(1, N, 8), cols, i32(1), f64(4), f64(1, 8, D), f64(1, 8))
    with pytest.raises(ValueError, match="do not match"):
        ops.logreg_batch_logits(Xd, f64(1, 8, D), None, cols, i32(2), f64(1, N, 8))
    with pytest.raises(ValueError, match="classes"):
        ops.logreg_columns([9])


# ---- the tool -----------------------------------------------------------------------------------------------------------------
def test_tool_end_to_end_with_the_lockstep_solver(tmp_path):
    spec = importlib.util.spec_from_file_location("sm3_logreg_cli_lockstep", os.path.join(TOOLS, "backbone_logreg.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    outs = []
    for run in ("a", "b"):
        log = tmp_path / run
        stat = tool.main(["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "--log-path", str(log),
                          "--random-features", "96", "40", "64", "--logreg-c", "0.01", "1", "100", "--save-features",
                          "--logreg-solver", "lockstep"])
        assert stat["problems"] == 24 and stat["not_converged"] == 0 and 0.0 <= stat["AUC_AVG"] <= 1.0
        outs.append(torch.load(log / "logreg_predictions.pt", weights_only=False))
    a, b = outs
    assert a["solver"] == b["solver"] == "lockstep"
    for x, y in zip(a["preds"], b["preds"]):
        assert torch.equal(x, y)
    assert a["C"] == b["C"] and torch.equal(a["selection"]["val_auc"], b["selection"]["val_auc"])
    for k in ("status", "iterations", "objective", "grad_norm"):
        assert torch.equal(a["status"][0][k], b["status"][0][k]), k
    sa = torch.load(tmp_path / "a" / "best_linear.pth", weights_only=False)["state_dict"]
    sb = torch.load(tmp_path / "b" / "best_linear.pth", weights_only=False)["state_dict"]
    assert sorted(sa) == sorted(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    # best_linear.pth on the saved features gives the saved logits to fp32 rounding -- of a 64-term dot product of magnitudes
    # |w| |x|, of the weights and of the features' scaling -- as the workgroup solver's tool test has it
    x = a["test_features"]
    for t in range(8):
        wt, bias = sa[f"classifier.{t}.weight"], sa[f"classifier.{t}.bias"]
        got = torch.nn.functional.linear(x, wt, bias).double()
        tol = 4 * (64 + 2) * 2.0 ** -24 * float((wt.abs().double() @ x.abs().double().T).max() + 1)
        err = float((got - a["preds"][t]).abs().max())
        print(f"label {t}: heads on the saved features against the saved logits {err:.2e} (<= {tol:.2e})")
        assert err <= tol, (t, err, tol)
