"""Shared inputs and the fp64 numpy restatement of the logistic-regression probe (sm3hip/logreg.py, csrc/logreg.hip), for
tests/test_logreg_cpu.py and tests/test_logreg_gpu.py.

The restatement states the problem once more, independently of the code under test:

    F(W, b) = (1 / S) sum_i s_i CE(softmax(W x_i + b), y_i) + (1 / (2 C S)) |W|^2,   S = sum_i s_i,

over the classes of positive total weight (a class without weight leaves the softmax: coefficient row 0, intercept -inf).  Its
optimum is found by scipy's L-BFGS-B and then polished by Newton steps (Hessian products, conjugate gradients), so its gradient norm is at rounding
level; test_logreg_cpu.py pins its probabilities to scikit-learn's.  It is the reference of the GPU tests: never the kernels.
"""
import numpy as np

NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]
LABELS = (2, 1, 0)                     # BWV (2 classes), PN (3), DIAG (5)
PARITY_CS = (0.01, 1.0, 100.0)
SHAPES = ((2, 1), (3, 5), (17, 33), (65, 130), (130, 515), (130, 1), (17, 515))   # (N, D)
Q = 12                                 # held-out rows per case

# The probability gap |restatement - scikit-learn| on held-out rows, the maximum over every case of test_logreg_cpu.py's parity
# tests (SHAPES x LABELS, plain / balanced / fold / multiplicity / zero-weight class), measured with scikit-learn 1.7.2
# (LogisticRegression(solver="lbfgs", tol=1e-10, max_iter=10000)) -- the figure, and the bound = 4 x the figure.  The gap is
# scikit-learn's own stopping error: it grows with C as the problem loses conditioning.
MEASURED_GAP = {0.01: 8.27e-7, 1.0: 2.84e-6, 100.0: 4.59e-5}
PARITY_BOUND = {c: 4.0 * g for c, g in MEASURED_GAP.items()}


def make_case(N, D, seed=0):
    """(X [N, D] float32, targets [N, 8] int64, Xq [Q, D] float32): standard normal features; a label is the argmax of a random
    linear map of the features plus noise, so it is learnable and not separable at small D.  The first two cases get the classes
    0 and 1 of every label, so that every label has two classes present at N = 2."""
    rs = np.random.RandomState(1000 * N + D + seed)
    X = rs.randn(N, D).astype(np.float32)
    Xq = rs.randn(Q, D).astype(np.float32)
    targets = np.zeros((N, 8), dtype=np.int64)
    for t, n in enumerate(NUM_CLASSES):
        A = rs.randn(D, n) / np.sqrt(D)
        targets[:, t] = np.argmax(X.astype(np.float64) @ A + 0.5 * rs.randn(N, n), axis=1)
        targets[0, t], targets[1, t] = 0, 1
    return X, targets, Xq


def present_classes(y, s, nt):
    cw = np.bincount(y, weights=s, minlength=nt)[:nt]
    return cw > 0


def balanced(s, y, nt):
    """scikit-learn's class_weight="balanced" under sample weights: s_i S / (n_present S_class(y_i))."""
    cw = np.bincount(y, weights=s, minlength=nt)[:nt]
    pres = cw > 0
    scale = np.where(pres, s.sum() / (pres.sum() * np.where(pres, cw, 1.0)), 0.0)
    return s * scale[y]


def value_and_grad(X, y, s, C, W, b, nt):
    """(F, grad_W [nt, D], grad_b [nt]) in fp64; the softmax runs over the classes of positive weight, the penalty over all rows."""
    X = np.asarray(X, dtype=np.float64)
    W, b = np.asarray(W, dtype=np.float64)[:nt], np.asarray(b, dtype=np.float64)[:nt]
    pres = present_classes(y, s, nt)
    S = s.sum()
    lam = 1.0 / (C * S)
    z = X @ W.T + np.where(pres, b, 0.0)
    z = np.where(pres, z, -np.inf)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    p = e / e.sum(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(e.sum(axis=1))
    act = s > 0
    zy = np.where(act, z[np.arange(len(y)), np.where(act, y, np.argmax(pres))], 0.0)
    F = float((s * np.where(act, lse - zy, 0.0)).sum() / S + 0.5 * lam * (W * W).sum())
    onehot = np.zeros_like(p)
    onehot[np.arange(len(y)), y] = 1.0
    r = (s[:, None] * (p - onehot)) / S
    r[~act] = 0.0
    r[:, ~pres] = 0.0
    return F, r.T @ X + lam * W, r.sum(axis=0)


def fit_ref(X, y, s, C, nt, gtol=1e-10, max_iter=1000):
    """The optimum in fp64: scipy L-BFGS-B from zero on the present classes, then Newton-CG steps until
    |grad|_inf <= gtol.  Returns dict(W [nt, D], b [nt] (-inf for a class without weight), status "ok" / "one_class" /
    "not_converged", iterations (L-BFGS-B's), F, grad_norm)."""
    from scipy.optimize import minimize
    X64 = np.asarray(X, dtype=np.float64)
    D = X64.shape[1]
    pres = present_classes(y, s, nt)
    k = int(pres.sum())
    W, b = np.zeros((nt, D)), np.where(pres, 0.0, -np.inf)
    if k < 2:
        return dict(W=W, b=b, status="one_class", iterations=0, F=0.0, grad_norm=0.0)
    idx = np.flatnonzero(pres)

    def unpack(v):
        Wf, bf = np.zeros((nt, D)), np.zeros(nt)
        Wf[idx], bf[idx] = v[:k * D].reshape(k, D), v[k * D:]
        return Wf, bf

    def fg(v):
        F, gW, gb = value_and_grad(X64, y, s, C, *unpack(v), nt)
        return F, np.concatenate([gW[idx].ravel(), gb[idx]])

    r = minimize(fg, np.zeros(k * D + k), jac=True, method="L-BFGS-B",
                 options=dict(maxiter=max_iter, maxfun=20 * max_iter, gtol=gtol, ftol=0.0, maxcor=10, maxls=50))
    v = r.x
    F, g = fg(v)
    S, lam = s.sum(), 1.0 / (C * s.sum())
    act = s > 0
    Xa, sa = np.concatenate([X64[act], np.ones((act.sum(), 1))], axis=1), s[act] / S
    pen = np.concatenate([np.full(D, lam), [0.0]])
    for _ in range(20):                                  # Newton polish; H v by products with X, H p = g by conjugate gradients
        if np.abs(g).max() <= gtol:
            break
        Wf, bf = unpack(v)
        z = X64[act] @ Wf[idx].T + bf[idx]
        p = np.exp(z - z.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)

        def hess(V):                                     # V [k, D + 1]
            u = Xa @ V.T
            return ((p * (u - (p * u).sum(axis=1, keepdims=True))) * sa[:, None]).T @ Xa + V * pen

        G = np.concatenate([g[:k * D].reshape(k, D), g[k * D:, None]], axis=1)
        G[:, D] -= G[:, D].mean()                        # H is singular along the common intercept shift: stay orthogonal to it
        step, res = np.zeros_like(G), G.copy()
        q, rr = res.copy(), (res * res).sum()
        for _ in range(500):
            Hq = hess(q)
            qHq = (q * Hq).sum()
            if not qHq > 0.0:
                break
            al = rr / qHq
            step += al * q
            res -= al * Hq
            res[:, D] -= res[:, D].mean()
            r2 = (res * res).sum()
            if r2 <= 1e-24 * (G * G).sum():
                break
            q, rr = res + (r2 / rr) * q, r2
        v2 = v - np.concatenate([step[:, :D].ravel(), step[:, D]])
        F2, g2 = fg(v2)
        if np.abs(g2).max() < np.abs(g).max():
            v, F, g = v2, F2, g2
        else:
            break
    W, bb = unpack(v)
    gn = float(np.abs(g).max())
    return dict(W=W, b=np.where(pres, bb, -np.inf), status="ok" if gn <= max(gtol, 1e-12) else "not_converged",
                iterations=int(r.nit), F=float(F), grad_norm=gn)


def probs(W, b, Xq):
    """softmax(W xq + b) in fp64; a class of intercept -inf has probability 0."""
    z = np.asarray(Xq, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def sklearn_probs(X, y, s, C, nt, Xq, class_weight=None):
    """scikit-learn's probabilities [Q, nt] for the same problem: fitted on the rows of positive weight (a class without weight
    is dropped, its column is 0), at 2 C when two classes remain (scikit-learn fits one sigmoid logit there)."""
    from sklearn.linear_model import LogisticRegression
    act = s > 0
    k = len(np.unique(y[act]))
    m = LogisticRegression(C=2.0 * C if k == 2 else C, solver="lbfgs", tol=1e-10, max_iter=10000, class_weight=class_weight)
    m.fit(np.asarray(X, dtype=np.float64)[act], y[act], sample_weight=s[act])
    out = np.zeros((len(Xq), nt))
    out[:, m.classes_] = m.predict_proba(np.asarray(Xq, dtype=np.float64))
    return out


def weight_rows(N, seed=0):
    """[4, N] fp64: all ones; a 0/1 fold row; integer multiplicities 0 .. 3; a row without weight on the cases of class 1 of
    label PN (so that PN loses a class).  The first two cases keep weight in every row but the last's class-1 cases."""
    rs = np.random.RandomState(77 + N + seed)
    fold = (rs.rand(N) < 0.7).astype(np.float64)
    mult = rs.randint(0, 4, N).astype(np.float64)
    fold[:2], mult[:2] = 1.0, 2.0
    return np.stack([np.ones(N), fold, mult, np.ones(N)])


def value_grad_bound(X, s, C, W, b, nt):
    """The rounding bound of F and of every gradient entry when only the summation ORDER differs (fp64, u = 2^-53).  A logit is a
    sum of D + 1 terms: |dz| <= (D + 2) u (|x| . |w| + |b|) =: ez.  The softmax and the log-sum-exp are 1-Lipschitz in the
    logits (sup norm, factor 2 for p), plus a few u for exp / log / the division: |dp| <= 2 ez + 8 u, |dCE| <= 2 ez + 8 u (|z| + 1).
    F is a weighted mean of N such terms (another (N + 2) u relative) plus the penalty (D nt + 2 terms).  A gradient entry
    sum_i r_ic x_ik has per-term error |x| |dp| s_i / S and summation error (N + 2) u sum |r x|; with |r_ic| <= s_i / S the sum
    of |r x| is at most max|x|.  Returns (bound_F, bound_grad), both scalars, doubled for slack in the elementary functions."""
    u = 2.0 ** -53
    X64 = np.abs(np.asarray(X, dtype=np.float64))
    N, D = X64.shape
    Wa, ba = np.abs(np.asarray(W, dtype=np.float64)[:nt]), np.abs(np.where(np.isfinite(b[:nt]), b[:nt], 0.0))
    zmag = (X64 @ Wa.T + ba).max() if N else 0.0
    ez = (D + 2) * u * zmag
    xmax = X64.max()
    lam = 1.0 / (C * s.sum())
    lam_w = lam * (Wa * Wa).sum()
    bF = 2.0 * ((2 * ez + 8 * u * (zmag + 1)) + (N + 2) * u * (2 * zmag + np.log(max(nt, 2))) + (D * nt + 4) * u * lam_w)
    bG = 2.0 * (xmax * (2 * ez + 8 * u) + (N + 2) * u * xmax + 4 * u * lam * Wa.max() + (N + 2) * u)
    return bF, bG


# ---- the problems both test files use ---------------------------------------------------------------------------------------
ROW_KINDS = ("ones", "fold", "multiplicity", "no_class_1")
ALL_ROW_SHAPES = ((17, 33), (65, 130))     # the shapes fitted with all four weight rows; the others with "ones" alone


def case_rows(N, targets):
    """weight_rows(N) with the last row's weight taken from every case of class 1 of label PN: there PN keeps classes 0 and 2
    (its class 1 leaves the softmax), BWV, whose cases of class 1 are other cases, keeps both of its classes or loses one."""
    rows = weight_rows(N)
    rows[3][targets[:, 1] == 1] = 0.0
    return rows


def rows_of(shape):
    return (0, 1, 2, 3) if tuple(shape) in ALL_ROW_SHAPES else (0,)


_REFERENCE = {}


def reference(N, D):
    """{(label, row, C): dict(fit_ref's keys, probs [Q, n_t] on the held-out rows)} of the problems of shape (N, D): LABELS x
    rows_of x PARITY_CS.  Computed once a session and left unchanged."""
    if (N, D) not in _REFERENCE:
        X, T, Xq = make_case(N, D)
        rows, out = case_rows(N, T), {}
        for t in LABELS:
            for r in rows_of((N, D)):
                for C in PARITY_CS:
                    f = fit_ref(X, T[:, t], rows[r], C, NUM_CLASSES[t])
                    f["probs"] = probs(f["W"], f["b"], Xq) if f["status"] != "one_class" else None
                    out[(t, r, C)] = f
        _REFERENCE[(N, D)] = out
    return _REFERENCE[(N, D)]
