"""Shared by tests/test_signif_cpu.py and tests/test_signif_gpu.py: the cases and the by-definition restatements of
sm3hip/significance.py and csrc/signif.hip.  Nothing here calls the module under test; numpy, Python integers and Fractions only
(torch for the fp64 softmax, the one expression the scores are defined by).

  * cases: integer-valued logits in {-1, 0, 1}, so scores tie within and across the two models; b == a; b = a with the columns
    of one label permuted; an independent b; labels with an empty class (P = 0) and a one-case class (P = 1);
  * swap bits from the Philox restatement of tests/test_report_cpu.py, stream 5;
  * counts by definition: the swapped predictions A', B' of a replicate are FORMED, then recounted with no joint ranking: A2 by
    the O(P Q) psi matrix (small N) or by searchsorted on the sorted negatives (large N), TP / FP from the swapped argmax;
  * placements by the psi matrix; DeLong by the Fraction formulas of the issue; McNemar by a direct binomial sum."""
import importlib.util
import math
import os
from fractions import Fraction

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]
PAIRS = [(t, c) for t, n in enumerate(NUM_CLASSES) for c in range(n)]
PSI_LIMIT = 600  # cases up to which A2 is counted by the O(P Q) matrix


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_REPORT_REF = None


def report_ref():
    """tests/test_report_cpu.py: philox4x32_10, counts, restated_inputs."""
    global _REPORT_REF
    if _REPORT_REF is None:
        _REPORT_REF = _load("sm3_signif_report_ref", os.path.join(ROOT, "tests", "test_report_cpu.py"))
    return _REPORT_REF


# ---- cases ------------------------------------------------------------------------------------------------------------------
def make_pair(N, kind, seed):
    """(a, b, targets): a, b 8 x [N, n_t] float32 with integer values in {-1, 0, 1}, targets [N, 8] int64.
    kind: "same" b == a; "permuted" b = a with the columns of label 0 rotated; "other" b drawn on its own; "sparse" as "other"
    with class 1 of every label empty (P = 0) and class 2 of the labels that have one held by case 0 alone (P = 1)."""
    g = torch.Generator().manual_seed(seed)
    targets = torch.stack([torch.randint(0, n, (N,), generator=g) for n in NUM_CLASSES], dim=1)
    a = [torch.randint(-1, 2, (N, n), generator=g).float() for n in NUM_CLASSES]
    if kind == "same":
        b = [p.clone() for p in a]
    elif kind == "permuted":
        b = [p.clone() for p in a]
        b[0] = a[0].roll(1, dims=1)
    else:
        b = [torch.randint(-1, 2, (N, n), generator=g).float() for n in NUM_CLASSES]
    if kind == "sparse":
        targets[targets == 1] = 0
        targets[targets == 2] = 0
        for t, n in enumerate(NUM_CLASSES):
            if n > 2:
                targets[0, t] = 2
    return a, b, targets


def scores(preds):
    """[24, N] fp64 numpy: softmax(logits.double(), 1) column by column."""
    return torch.cat([torch.softmax(p.double(), dim=1).t() for p in preds], dim=0).numpy()


def argmax(preds):
    """[N, 8] int64: the lowest index of the row maximum."""
    return np.stack([p.double().numpy().argmax(axis=1) for p in preds], axis=1).astype(np.int64)


# ---- swap bits --------------------------------------------------------------------------------------------------------------
def swap_bits(seed, r, N):
    """[N] bool: bit i & 31 of word i >> 5; word d = word d % 4 of Philox4x32-10 with key = the seed, counter (d // 4, r, 0, 5)."""
    ref = report_ref()
    W = (N + 31) // 32
    q = np.arange((W + 3) // 4, dtype=np.uint64)
    w = np.stack(ref.philox4x32_10(q, np.uint64(r), np.uint64(0), np.uint64(5), seed & 0xFFFFFFFF, seed >> 32), axis=1).reshape(-1)
    return np.array([(int(w[i >> 5]) >> (i & 31)) & 1 for i in range(N)], dtype=bool)


# ---- counts by definition ---------------------------------------------------------------------------------------------------
def a2_by_definition(s, pos):
    """2 * #{(i, j): s_i > s_j} + #{s_i == s_j} over positives i and negatives j."""
    x, y = s[pos], s[~pos]
    if x.size == 0 or y.size == 0:
        return 0
    if s.shape[0] <= PSI_LIMIT:
        return int(2 * (x[:, None] > y[None, :]).sum() + (x[:, None] == y[None, :]).sum())
    ys = np.sort(y)
    return int(np.searchsorted(ys, x, side="left").sum() + np.searchsorted(ys, x, side="right").sum())


def side_counts(s, yhat, y):
    """[24, 3] int64 (A2, TP, FP) of one set of scores s [24, N] and predicted classes yhat [N, 8]."""
    out = np.zeros((len(PAIRS), 3), dtype=np.int64)
    for k, (t, c) in enumerate(PAIRS):
        pos = y[:, t] == c
        out[k] = (a2_by_definition(s[k], pos), int((pos & (yhat[:, t] == c)).sum()), int((~pos & (yhat[:, t] == c)).sum()))
    return out


def recount(sa, sb, ha, hb, y, swap):
    """[24, 2, 3] int64: A' takes b's score and predicted class of the swapped cases and a's of the others, B' the rest."""
    s1, s2 = np.where(swap[None, :], sb, sa), np.where(swap[None, :], sa, sb)
    h1, h2 = np.where(swap[:, None], hb, ha), np.where(swap[:, None], ha, hb)
    return np.stack([side_counts(s1, h1, y), side_counts(s2, h2, y)], axis=1)


def full_counts(side, y):
    """[24, 2, 3] (A2, TP, FP) -> [2, 24, 6] (A2, P, Q, TP, FP, FN)."""
    out = np.zeros((2, len(PAIRS), 6), dtype=np.int64)
    for k, (t, c) in enumerate(PAIRS):
        P = int((y[:, t] == c).sum())
        for w in range(2):
            A2, TP, FP = (int(v) for v in side[k, w])
            out[w, k] = (A2, P, y.shape[0] - P, TP, FP, P - TP)
    return out


def joint_counts(sa, sb, ha, hb, y, swap):
    """The kernel's route in numpy: ONE joint stable ranking of the 2N scores per column (element 2 i + w), tie groups by ==, the
    prefix sums of each side's negatives, A2 = sum over the side's positives of S[gs] + S[ge]."""
    N = y.shape[0]
    out = np.zeros((len(PAIRS), 2, 3), dtype=np.int64)
    for k, (t, c) in enumerate(PAIRS):
        joint = np.stack([sa[k], sb[k]], axis=1).reshape(-1)
        order = np.argsort(joint, kind="stable")
        ss = joint[order]
        new = np.concatenate([[True], ss[1:] != ss[:-1]])
        gs = np.maximum.accumulate(np.where(new, np.arange(2 * N), 0))
        last = np.concatenate([ss[1:] != ss[:-1], [True]])
        ge = np.minimum.accumulate(np.where(last, np.arange(2 * N) + 1, 2 * N)[::-1])[::-1]
        case, w = order >> 1, order & 1
        side = w ^ swap[case].astype(np.int64)
        pos = y[case, t] == c
        hit = np.where(w == 1, hb[case, t], ha[case, t]) == c
        for sd in range(2):
            S = np.concatenate([[0], np.cumsum((~pos) & (side == sd))])
            mine = pos & (side == sd)
            out[k, sd] = (int((S[gs[mine]] + S[ge[mine]]).sum()), int((mine & hit).sum()), int((~pos & (side == sd) & hit).sum()))
    return out


# ---- DeLong by definition ---------------------------------------------------------------------------------------------------
def placements_by_psi(s, pos):
    """[N] int64 in case order: positives 2 * (negatives below) + tied negatives, negatives 2 * (positives above) + tied positives."""
    x, y = s[pos], s[~pos]
    psi2 = 2 * (x[:, None] > y[None, :]).astype(np.int64) + (x[:, None] == y[None, :]).astype(np.int64)
    out = np.zeros(s.shape[0], dtype=np.int64)
    out[pos], out[~pos] = psi2.sum(axis=1), psi2.sum(axis=0)
    return out


def delong_exact(ua, ub, va, vb):
    """(theta_a, theta_b, Var(theta_a - theta_b), Var_a, Var_b) as Fractions from the doubled placements; a variance is None
    when P < 2 or Q < 2."""
    ua, ub, va, vb = ([int(v) for v in x] for x in (ua, ub, va, vb))
    P, Q = len(ua), len(va)

    def var(x, y):
        if P < 2 or Q < 2:
            return None
        return (Fraction(P * sum(v * v for v in x) - sum(x) ** 2, 4 * Q * Q * P * P * (P - 1))
                + Fraction(Q * sum(v * v for v in y) - sum(y) ** 2, 4 * P * P * Q * Q * (Q - 1)))
    theta = [Fraction(sum(u), 2 * P * Q) if P * Q else Fraction(0) for u in (ua, ub)]
    d, e = [p - q for p, q in zip(ua, ub)], [p - q for p, q in zip(va, vb)]
    return theta[0], theta[1], var(d, e), var(ua, va), var(ub, vb)


def delong_z_p(theta_a, theta_b, var):
    """(z, p, undefined) by the issue's arithmetic: one rounding of each exact rational, erfc for the two-sided p."""
    if var is None or var == 0:
        return 0.0, 1.0, True
    z = float(theta_a - theta_b) / math.sqrt(float(var))
    return z, math.erfc(abs(z) / math.sqrt(2.0)), False


# ---- permutation p, McNemar, Holm -------------------------------------------------------------------------------------------
def permutation_p(t_point, t_reps):
    """(1 + #{r: |T_r| >= |T_point|}) / (B + 1), element-wise over [..] and [B, ..]."""
    t_point, t_reps = np.asarray(t_point, dtype=np.float64), np.asarray(t_reps, dtype=np.float64)
    return (1.0 + (np.abs(t_reps) >= np.abs(t_point)[None]).sum(axis=0)) / float(t_reps.shape[0] + 1)


def mcnemar_exact(n10, n01):
    n = n10 + n01
    if n == 0:
        return 1.0
    return float(min(Fraction(1), Fraction(2 * sum(math.comb(n, k) for k in range(min(n10, n01) + 1)), 2 ** n)))


def holm_by_definition(p):
    """Holm: the i-th smallest (ties by index) times (m - i), at most 1, made monotone."""
    p = [float(v) for v in p]
    m = len(p)
    idx = sorted(range(m), key=lambda k: (p[k], k))
    out, run = [0.0] * m, 0.0
    for i, k in enumerate(idx):
        run = max(run, min(1.0, (m - i) * p[k]))
        out[k] = run
    return np.array(out)


def placements_by_sort(s, pos):
    """placements_by_psi for the large N: searchsorted on the sorted negatives and positives."""
    x, y = s[pos], s[~pos]
    ys, xs = np.sort(y), np.sort(x)
    out = np.zeros(s.shape[0], dtype=np.int64)
    out[pos] = np.searchsorted(ys, x, side="left") + np.searchsorted(ys, x, side="right")
    left, right = np.searchsorted(xs, y, side="left"), np.searchsorted(xs, y, side="right")
    out[~pos] = 2 * (x.shape[0] - right) + (right - left)
    return out


# ---- a case with power ------------------------------------------------------------------------------------------------------
def power_case(N=200, seed=5):
    """a: integer logits that favour the true class (2 on it, plus noise in {-1, 0, 1}); b: a noisy copy of a (noise in
    {-3 .. 3} added), so b ranks clearly worse.  Integer-valued, so the scores still tie."""
    g = torch.Generator().manual_seed(seed)
    targets = torch.stack([torch.randint(0, n, (N,), generator=g) for n in NUM_CLASSES], dim=1)
    a, b = [], []
    for t, n in enumerate(NUM_CLASSES):
        p = 2.0 * torch.nn.functional.one_hot(targets[:, t], n).float() + torch.randint(-1, 2, (N, n), generator=g).float()
        a.append(p)
        b.append(p + torch.randint(-3, 4, (N, n), generator=g).float())
    return a, b, targets


def restated_auc_test(a, b, targets, k, B, seed, score=scores):
    """(T_point, permutation p, DeLong z, DeLong p) of the AUC of column k, all by the restatements above.  score: preds ->
    [24, N] fp64 (the GPU tests pass the device's softmax, whose last bit, and so whose ties, may differ from the CPU's)."""
    t, c = PAIRS[k]
    sa, sb, y = score(a)[k], score(b)[k], targets.numpy()
    pos = y[:, t] == c
    P, Q = int(pos.sum()), int((~pos).sum())

    def stat(swap):
        s1, s2 = np.where(swap, sb, sa), np.where(swap, sa, sb)
        return a2_by_definition(s1, pos) / float(2 * P * Q) - a2_by_definition(s2, pos) / float(2 * P * Q)
    N = y.shape[0]
    point = stat(np.zeros(N, dtype=bool))
    reps = np.array([stat(swap_bits(seed, r, N)) for r in range(B)])
    pa, pb = placements_by_psi(sa, pos), placements_by_psi(sb, pos)
    ta, tb, var, _, _ = delong_exact(pa[pos], pb[pos], pa[~pos], pb[~pos])
    z, p, _ = delong_z_p(ta, tb, var)
    return point, float(permutation_p(point, reps)), z, p
