"""Seeded inputs and the restatement of the conformal report (sm3hip/conformal.py, csrc/conformal.hip) in Python integers and
numpy, shared by tests/test_conformal_cpu.py and tests/test_conformal_gpu.py.

The restatement is literal: every calibration case becomes w copies of its true-class score, the copies are sorted, the k-th is
taken (k from fractions.Fraction); the sets of the test split are counted one case at a time.  The multiplicities come from this
directory's own Philox (tests/test_report_cpu.py), with the last counter word as an argument: 2 for the test split, 6 for the
calibration split."""
import fractions
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]
PAIRS = [(t, c) for t, n in enumerate(NUM_CLASSES) for c in range(n)]
FIRST = [PAIRS.index((t, 0)) for t in range(8)]
ONE = 1 << 32
INF = 1 << 40
RECORD = 24


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REP = _load("sm3_conformal_report_ref", os.path.join(ROOT, "tests", "test_report_cpu.py"))  # philox4x32_10, make_case
make_case = REP.make_case


def multiplicities(seed, r, N, word):
    """[N] int64: draw d hits case (w * N) >> 32, w = word d % 4 of the call with counter (d // 4, r, 0, word)."""
    q = np.arange((N + 3) // 4, dtype=np.uint64)
    w = np.stack(REP.philox4x32_10(q, np.uint64(r), np.uint64(0), np.uint64(word), seed & 0xFFFFFFFF, seed >> 32), axis=1)
    idx = (w.reshape(-1)[:N] * np.uint64(N)) >> np.uint64(32)
    return np.bincount(idx.astype(np.int64), minlength=N).astype(np.int64)


def fraction(alpha):
    return fractions.Fraction(str(alpha))


def rank(n, alpha):
    """k = ceil((n + 1)(1 - alpha)) in exact rationals."""
    f = (n + 1) * (1 - fraction(alpha))
    return -((-f.numerator) // f.denominator)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def case(N, kind, seed):
    """tests/test_report_cpu.py's make_case ("ties", "equal", "absent", "random") with, for every kind but "equal", rows certain
    of one class in: q = 2^32 and q = 0."""
    preds, targets = make_case(N, kind, seed)
    if kind != "equal":
        for t, p in enumerate(preds):
            p[::7, t % p.shape[1]] = 2000.0
    return preds, targets


def sampled_split(N, g, classes=5, scale=2.0):
    """Logits scale * N(0, 1) with `classes` classes and labels drawn from their own softmax by the numpy Generator g: (logits
    [N, classes] fp64, y [N])."""
    z = scale * g.standard_normal((N, classes))
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    y = (g.random(N)[:, None] > np.cumsum(p, axis=1)).sum(axis=1).clip(0, classes - 1)
    return z, y


# ---- the restatement -----------------------------------------------------------------------------------------------------
def q32(preds, temperature=None):
    """q [24, N] int64 through the library's own fixed_point (the class-wise series), on the tensors' device."""
    from sm3hip import calibration
    N = preds[0].shape[0]
    q = calibration.fixed_point(preds, torch.zeros((N, 8), dtype=torch.int64, device=preds[0].device), temperature)[0][8:]
    return q.cpu().numpy().astype(np.int64)


def scores_of_row(q, method):
    """The scores of one label's classes for one case: q a list of Python ints."""
    if method == "lac":
        return [ONE - v for v in q]
    return [sum(q[d] for d in range(len(q)) if q[d] > q[c] or (q[d] == q[c] and d <= c)) for c in range(len(q))]


def scores(q, method):
    """s [24, N] int64 from q [24, N], one (case, label) at a time."""
    q = np.asarray(q, dtype=np.int64)
    out = np.zeros(q.shape, dtype=np.int64)
    for t, n in enumerate(NUM_CLASSES):
        rows = q[FIRST[t]:FIRST[t] + n].T.tolist()                      # Python ints
        out[FIRST[t]:FIRST[t] + n] = np.array([scores_of_row(row, method) for row in rows], dtype=np.int64).reshape(-1, n).T
    return out


def true_scores(s, y):
    """a [8, N]: a[t, n] = s[column (t, y_n), n]."""
    y = np.asarray(y, dtype=np.int64)
    return np.stack([s[FIRST[t] + y[:, t], np.arange(y.shape[0])] for t in range(8)])


def copies(a, w):
    """Every case w times, sorted: a list of Python ints."""
    return sorted(np.repeat(np.asarray(a, dtype=np.int64), np.asarray(w, dtype=np.int64)).tolist())


def kth(a, w, alpha):
    """The threshold of the scores a [n] with multiplicities w [n] at the level alpha: every case w times, sorted, the k-th."""
    c = copies(a, w)
    k = rank(len(c), alpha)
    return INF if k > len(c) else c[k - 1]


def thresholds(cal_a, cal_y, w, alphas, conditional):
    """thr [8, A, 5] int64 (0 in the slots of classes a label lacks)."""
    cal_a, cal_y, w = np.asarray(cal_a), np.asarray(cal_y), np.asarray(w)
    out = np.zeros((8, len(alphas), 5), dtype=np.int64)
    for t, n in enumerate(NUM_CLASSES):
        for c in range(n):
            sel = np.ones(len(w), dtype=bool) if conditional == "marginal" else cal_y[:, t] == c
            srt = copies(cal_a[t][sel], w[sel])                          # sorted once for all the levels
            for a, alpha in enumerate(alphas):
                k = rank(len(srt), alpha)
                out[t, a, c] = INF if k > len(srt) else srt[k - 1]
    return out


def records(s, y, m, thr):
    """counts [8, A, 24] int64 of the test scores s [24, N], classes y [N, 8] and multiplicities m [N] under thr [8, A, 5]."""
    A = thr.shape[1]
    out = [[[0] * RECORD for _ in range(A)] for _ in range(8)]
    for i in range(len(m)):
        mi = int(m[i])
        if not mi:
            continue
        for t, n in enumerate(NUM_CLASSES):
            yi = int(y[i][t])
            for a in range(A):
                rec = out[t][a]
                inset = [int(s[FIRST[t] + c][i]) <= int(thr[t][a][c]) for c in range(n)]
                size = sum(inset)
                covered = 0 <= yi < n and inset[yi]
                rec[0] += mi * covered
                rec[1] += mi * size
                rec[2] += mi * (covered and size == 1)
                rec[3 + size] += mi
                for c in range(n):
                    rec[9 + 3 * c] += mi * (yi == c)
                    rec[10 + 3 * c] += mi * (yi == c and inset[c])
                    rec[11 + 3 * c] += mi * inset[c]
    return np.array(out, dtype=np.int64)


def records_np(s, y, m, thr):
    """records, a (label, level) at a time over all cases: for the sizes at which the loop above takes minutes.
    tests/test_conformal_cpu.py holds it to records."""
    s, y, m, thr = (np.asarray(v, dtype=np.int64) for v in (s, y, m, thr))
    out = np.zeros((8, thr.shape[1], RECORD), dtype=np.int64)
    for t, n in enumerate(NUM_CLASSES):
        hit = y[:, t][None, :] == np.arange(n)[:, None]                                  # [n, N]
        for a in range(thr.shape[1]):
            inset = s[FIRST[t]:FIRST[t] + n] <= thr[t, a, :n, None]
            size, covered = inset.sum(axis=0), (inset & hit).any(axis=0)
            out[t, a, 0], out[t, a, 1], out[t, a, 2] = m[covered].sum(), (m * size).sum(), m[covered & (size == 1)].sum()
            for k in range(6):
                out[t, a, 3 + k] = m[size == k].sum()
            for c in range(n):
                out[t, a, 9 + 3 * c:12 + 3 * c] = m[hit[c]].sum(), m[hit[c] & inset[c]].sum(), m[inset[c]].sum()
    return out


class Restated:
    """The score tables of a pair of splits, computed once, for many multiplicities."""

    def __init__(self, cal, test, method, temperature=None):
        self.cal_s, self.s = scores(q32(cal[0], temperature), method), scores(q32(test[0], temperature), method)
        self.cal_y, self.y = cal[1].cpu().numpy(), test[1].cpu().numpy()
        self.cal_a = true_scores(self.cal_s, self.cal_y)

    def __call__(self, alphas, conditional, w=None, m=None, fixed=None):
        w = np.ones(self.cal_y.shape[0], dtype=np.int64) if w is None else w
        m = np.ones(self.y.shape[0], dtype=np.int64) if m is None else m
        thr = thresholds(self.cal_a, self.cal_y, w, alphas, conditional) if fixed is None else np.asarray(fixed)
        return (records if len(m) <= 64 else records_np)(self.s, self.y, m, thr), thr


def restate(cal, test, alphas, method, conditional, w=None, m=None, temperature=None, fixed=None):
    """(counts [8, A, 24], thr [8, A, 5]) of the splits cal = (preds, targets) and test = (preds, targets); w, m: the
    multiplicities (None: all 1); fixed: thresholds to count under instead of fitting."""
    return Restated(cal, test, method, temperature)(alphas, conditional, w, m, fixed)


def values(counts, thr, N):
    """(label [A][5][9], class coverage and inclusion [A][2][24], thresholds [A][8][5]) in Python numbers: ONE division each."""
    A = len(counts[0])
    label, cls, tv = [], [], []
    for a in range(A):
        rows = [[], [], [], [], []]
        for t in range(8):
            r = [int(v) for v in counts[t][a]]
            for i, (num, den) in enumerate(((r[0], N), (r[1], N), (r[3], N), (r[4], N), (r[2], r[4]))):
                rows[i].append(float(num) / float(den) if den else 0.0)
        for row in rows:
            acc = 0.0
            for v in row[:8]:
                acc = acc + v
            row.append(acc / 8.0)
        label.append(rows)
        cc, inc = [], []
        for t, c in PAIRS:
            r = [int(v) for v in counts[t][a]]
            cc.append(float(r[10 + 3 * c]) / float(r[9 + 3 * c]) if r[9 + 3 * c] else 0.0)
            inc.append(float(r[11 + 3 * c]) / float(N))
        cls.append([cc, inc])
        tv.append([[float("inf") if int(thr[t][a][c]) >= INF else float(int(thr[t][a][c])) / float(ONE) for c in range(5)]
                   for t in range(8)])
    return label, cls, tv
