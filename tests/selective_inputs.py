"""Seeded inputs and the restatement of the selective-prediction report (sm3hip/selective.py, csrc/selective.hip) in Python
integers, shared by tests/test_selective_cpu.py and tests/test_selective_gpu.py.

The restatement is literal: a replicate becomes its copies in ranking order, the copies are walked one at a time with running
counters, an error copy at rank r adds the table's tail t[r] = PH[r] - PH[r - 1] to A.  The multiplicities come from this
directory's own Philox (tests/test_report_cpu.py) on stream word 2."""
import fractions
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]
CLS_WEIGHTS = [2, 2, 1, 2, 2, 2, 2, 1]
KINDS = ("random", "ties", "equal", "no_errors", "all_errors", "errors_last", "errors_first")
ONE = 1 << 32


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REP = _load("sm3_selective_report_ref", os.path.join(ROOT, "tests", "test_report_cpu.py"))  # philox4x32_10, make_case
make_case = REP.make_case


def words(n, seed, r, word):
    """n Philox words (uint64 array of 32-bit values): word d = word d % 4 of the call with counter (d // 4, r, 0, word)."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    w = np.stack(REP.philox4x32_10(q, np.uint64(r), np.uint64(0), np.uint64(word), seed & 0xFFFFFFFF, seed >> 32), axis=1)
    return w.reshape(-1)[:n]


def multiplicities(seed, r, N, word=2):
    """[N] int64: draw d hits case (w * N) >> 32."""
    idx = (words(N, seed, r, word) * np.uint64(N)) >> np.uint64(32)
    return np.bincount(idx.astype(np.int64), minlength=N).astype(np.int64)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def case(N, kind, seed):
    """preds (8 x [N, n_t] float32) and targets [N, 8] int64.  "random", "ties" (integer logits: few distinct keys, big groups)
    and "equal" (one group) are make_case's; "no_errors" / "all_errors" set the targets to / off the predicted class;
    "errors_last" / "errors_first": the predicted class leads the others (all 0) by a gap that is different for every case, in
    an order drawn from Philox, and the quarter of the cases with the smallest / largest gaps is wrong -- a perfect ranking and
    its opposite, under every score."""
    if kind in ("random", "ties", "equal"):
        return make_case(N, kind, seed)
    preds, targets = make_case(N, "random", seed)
    if kind in ("errors_last", "errors_first"):
        for t, n in enumerate(NUM_CLASSES):
            rank = np.argsort(np.argsort(words(N, seed, t, 0), kind="stable"), kind="stable")          # a permutation of 0 .. N - 1
            cls = (words(N, seed, t, 1) % np.uint64(n)).astype(np.int64)
            p = torch.zeros(N, n)
            p[torch.arange(N), torch.from_numpy(cls)] = torch.from_numpy(0.5 + 0.001 * rank).float()
            preds[t] = p
            wrong = rank < N // 4 if kind == "errors_last" else rank >= N - N // 4
            targets[:, t] = torch.from_numpy(np.where(wrong, (cls + 1) % n, cls))
        return preds, targets
    for t, n in enumerate(NUM_CLASSES):
        yhat = preds[t].argmax(dim=1)
        targets[:, t] = yhat if kind == "no_errors" else (yhat + 1) % n
    return preds, targets


def flags(preds, targets):
    """(err, pos, call) [8, N] bool in numpy: yhat = the lowest index of the row maximum."""
    y = targets.cpu().numpy()
    yhat = np.stack([p.cpu().numpy().argmax(axis=1) for p in preds], axis=1)
    sel = np.array(CLS_WEIGHTS)[None, :]
    return (yhat != y).T, (y == sel).T, (yhat == sel).T


def ranked(preds, targets, score="msp", temperature=None):
    """(order [8, N], last [8, N] by sorted position, sorted keys [8, N], ties [8]) as numpy, through the library's own keys and
    ranking (torch plumbing, which tests/test_selective_cpu.py holds to a literal sort) on the tensors' device."""
    from sm3hip import selective
    key = selective.keys(preds, score, temperature)
    msp = selective.keys(preds, "msp", temperature)
    order, last, ties, ks = selective.ranking(key, msp)
    return order.cpu().numpy().astype(np.int64), last.cpu().numpy(), ks.cpu().numpy(), ties.cpu().numpy()


# ---- the restatement -----------------------------------------------------------------------------------------------------
def tails(N):
    """t[1 .. N] of the harmonic-tail table in Python integers (t[0] unused), and PH [N + 1]."""
    f, t = 0, [0] * (N + 2)
    for k in range(N, 0, -1):
        f = f + (1 << 64) // k
        t[k] = (f + (1 << 31)) >> 32
    ph = [0]
    for r in range(1, N + 1):
        ph.append(ph[-1] + t[r])
    return t, ph


def label_record(order, err, pos, call, last, m, tail, kcuts, risks, pcuts):
    """The record of one label as a list of Python ints, and the error count after every copy (for the exact AURC)."""
    N = len(order)
    C = E = P = TP = FP = FN = A = 0
    cov = {}
    best = [(0, 0)] * len(risks)
    before = []
    curve = []
    for j in range(N):
        n = int(order[j])
        before.append((C, E, TP, FP, FN))
        for _ in range(int(m[n])):                      # the copies of the case, one at a time
            C += 1
            e, p, c = bool(err[n]), bool(pos[n]), bool(call[n])
            E += e
            P += p
            TP += c and p
            FP += c and not p
            FN += p and not c
            if e:
                A += tail[C]
            cov[C] = (E, TP, FP, FN)
            curve.append(E)
        if last[j] and C >= 1:
            for h, (a, b) in enumerate(risks):
                if E * b <= a * C:
                    best[h] = (C, E)                    # C only grows: the last that qualifies is the largest
    before.append((C, E, TP, FP, FN))
    rec = [A, E, P]
    for k in kcuts:
        rec += list(cov[k])
    for cut in best:
        rec += list(cut)
    for p in pcuts:
        rec += list(before[p])
    return [int(v) for v in rec], curve


def records(order, flg, last, m, kcuts, risks, pcuts):
    """[8, R] int64: the records of the 8 labels under the multiplicities m [N] (None: all 1); pcuts [8][Pc]."""
    N = order.shape[1]
    m = np.ones(N, dtype=np.int64) if m is None else m
    tail, _ = tails(N)
    err, pos, call = flg
    return np.array([label_record(order[t], err[t], pos[t], call[t], last[t], m, tail, kcuts, risks, pcuts[t])[0]
                     for t in range(8)], dtype=np.int64)


def exact_aurc(order, err, m=None):
    """The exact Fraction (1 / N) sum_{k = 1 .. N} err(k) / k of one label."""
    N = len(order)
    m = np.ones(N, dtype=np.int64) if m is None else m
    _, curve = label_record(order, err, err, err, np.zeros(N, dtype=bool), m, [0] * (N + 2), [], [], [])
    return sum(fractions.Fraction(e, k + 1) for k, e in enumerate(curve)) / N


def levels(N, G, H, Pc, seed=0):
    """Levels at their limits for N cases: (kcuts [G] with 1 and N, risks [H] pairs with 0 / 1 and 1 / 1, pcuts [8][Pc] with 0 and
    N); the rest drawn from Philox."""
    w = words(G + 2 * H + 8 * Pc, seed, 77, 0).astype(np.int64)
    kcuts = ([1, N] + [1 + int(v) % N for v in w[:G]])[:G]
    risks = ([(0, 1), (1, 1)] + [(int(a) % 21, 20) for a in w[G:G + H]])[:H]
    pcuts = [([0, N] + [int(v) % (N + 1) for v in w[G + 2 * H + t * Pc:G + 2 * H + (t + 1) * Pc]])[:Pc] for t in range(8)]
    return kcuts, risks, pcuts
