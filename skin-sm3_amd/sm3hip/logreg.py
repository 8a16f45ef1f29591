"""L-BFGS logistic-regression probe on cached encoder features (csrc/logreg.hip): the "linear probe" of the
self-supervised-learning papers -- frozen features once, an L2-regularised multinomial logistic regression fitted to its
optimum, C swept and picked on held-out cases.

THE PROBLEM.  p = (label t, C, weight row s): t one of the 8 derm7pt labels with n_t = NUM_CLASSES[t] classes, s one weight
s_i >= 0 per training row; every problem fits the same N rows of one feature matrix X [N, D] float32.  With S = sum_i s_i and
lambda = 1 / (C S),

    F(W, b) = (1 / S) sum_i s_i CE(softmax(W x_i + b), y_it) + (lambda / 2) |W|_F^2        (b is not penalised)

whose minimiser is that of scikit-learn's LogisticRegression(C=C, solver="lbfgs") with sample_weight=s (for a two-class label
scikit-learn fits one sigmoid logit: the two-class softmax equals it at C_sklearn = 2 C).  Folds and label fractions are 0/1
rows, class_weight="balanced" multiplies s_i by S / (n_present S_class(y_i)), bootstrap multiplicities are integer rows.  A
class of zero total weight leaves the softmax (coefficient row 0, intercept -inf, probability 0); a problem with fewer than two
classes of positive weight is not fitted (STATUS "one_class").  The softmax is shift-invariant in b: intercepts are defined up
to a constant per problem.

One workgroup fits one problem, so the result of a problem is a function of (X, y_t, s, C, gtol, max_iter) alone: equal in bits
alone or in any batch, at any position, for any `chunk`, on repeated calls.  Everything but X is fp64.  A launch runs a bounded
number of iterations (launch_iterations) and saves the solvers' state; the host reads the statuses and launches again until every
problem has finished -- the result does not depend on where the launches are cut.

TWO SOLVERS of the same problems, by the same L-BFGS rules.  solver="workgroup" (the default) is the one above.
solver="lockstep" takes the problems of a chunk through every iteration side by side: the two passes over X of an iteration are
two products on the f64 MFMA that all problems share -- one [N, D] x [D, columns] product for the logits, one [columns, N] x
[N, D] product for the gradients, a column being one (problem, class) pair -- and the per-problem steps run between them.  Its
sums run in other orders than the workgroup solver's, so the two agree to rounding and to the stopping tolerance, not in bits;
each keeps the bits contract above for itself.
"""
import math

import numpy as np
import torch

from . import ops, resample
from .metrics import CLS_WEIGHTS, NUM_CLASSES, multiclass_auroc

MAX_ROWS = ops.LOGREG_MAX_ROWS
MAX_DIM = ops.LOGREG_MAX_DIM
MAX_CLASSES = ops.LOGREG_MAX_CLASSES
STATUS = ("ok", "max_iter", "no_step", "one_class", "bad_entry")
SOLVERS = ("workgroup", "lockstep")
DEFAULT_CS = tuple(float(c) for c in np.logspace(-4, 4, 16))
NORMALIZE = ("none", "l2", "standardize")
WORKSPACE_BYTES = 2 << 30  # what the default chunk keeps a launch's workspace under
_FOLD_STREAM, _FRACTION_STREAM = 3, 4


# ---- the arguments ------------------------------------------------------------------------------------------------------------
def _features(X, who, name="X"):
    if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError(f"{who}: {name} must be a 2-D float32 tensor")
    if not 1 <= X.shape[0] <= MAX_ROWS and name == "X":
        raise ValueError(f"{who}: {X.shape[0]} rows, 1 to MAX_ROWS = {MAX_ROWS} are supported")
    if not 1 <= X.shape[1] <= MAX_DIM:
        raise ValueError(f"{who}: {X.shape[1]} features, 1 to MAX_DIM = {MAX_DIM} are supported")
    return X


def _host_targets(targets, N, who):
    t = torch.as_tensor(targets)
    if t.dim() != 2 or tuple(t.shape) != (N, len(NUM_CLASSES)) or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"{who}: targets must be an integer tensor [{N}, {len(NUM_CLASSES)}]")
    return t.detach().to("cpu", torch.int32).contiguous()


def _host_weights(weights, N, who):
    if weights is None:
        return torch.ones(1, N, dtype=torch.float64)
    w = torch.as_tensor(weights)
    if w.dim() == 1:
        w = w[None]
    if w.dim() != 2 or w.shape[1] != N or w.shape[0] < 1:
        raise ValueError(f"{who}: weights must be [R, {N}] (or [{N}])")
    return w.detach().to("cpu", torch.float64).contiguous()


def _host_problems(problems, who):
    out = []
    for e in problems:
        if len(e) != 3:
            raise ValueError(f"{who}: a problem is (label, C, weight row)")
        t, c, r = e
        if not resample.is_int(t) or not resample.is_int(r) or isinstance(c, bool) or not isinstance(c, (int, float)):
            raise ValueError(f"{who}: a problem is (label, C, weight row), got {e!r}")
        if not 0 <= t < len(NUM_CLASSES):
            raise ValueError(f"{who}: label {t} is not one of the {len(NUM_CLASSES)} labels")
        out.append((t, float(c), r))
    if not out:
        raise ValueError(f"{who}: no problem")
    return out


def _tables(problems):
    table = torch.tensor([[t, r, NUM_CLASSES[t], 0] for t, _, r in problems], dtype=torch.int32)
    return table, torch.tensor([c for _, c, _ in problems], dtype=torch.float64)


def _require_gpu(X, who):
    if not X.is_cuda:
        raise ValueError(f"{who}: the features must live on the GPU (the SM3 HIP path has no CPU fallback)")
    return X.contiguous()


def _solver(solver, who):
    if solver not in SOLVERS:
        raise ValueError(f"{who}: solver must be one of {SOLVERS}, got {solver!r}")
    return solver


def _pad_classes(t):
    """[P, n, ...] -> [P, 8, ...], zero rows behind."""
    if t.shape[1] == MAX_CLASSES:
        return t.contiguous()
    pad = torch.zeros((t.shape[0], MAX_CLASSES - t.shape[1]) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)
    return torch.cat([t, pad], dim=1).contiguous()


def balanced(weights, targets, label):
    """class_weight="balanced" of scikit-learn on the host rows `weights` [R, N] for one label: s_i S / (n_present S_class(y_i)),
    S and S_class the row's total and per-class weight, n_present its classes of positive weight.  fp64."""
    y = targets[:, label].long()
    out = weights.clone()
    for r in range(weights.shape[0]):
        s = weights[r]
        cls = torch.zeros(NUM_CLASSES[label], dtype=torch.float64).index_add_(0, y, s)
        present = int((cls > 0).sum())
        if present:
            scale = s.sum() / (present * cls)
            out[r] = s * torch.where(cls > 0, scale, torch.zeros_like(scale))[y]
    return out


# ---- value and gradient -------------------------------------------------------------------------------------------------------
def value_and_grad(X, targets, problems, W, b, weights=None, solver="workgroup"):
    """(F [P], grad_W [P, n, D], grad_b [P, n]) float64 of the problems [(label, C, weight row), ...] at W [P, n, D], b [P, n]
    (n >= the classes of every label named, at most 8): the certificate of any solution, scikit-learn's included -- at the
    optimum grad is 0.  An intercept of -inf is accepted for a class of zero weight.  solver: which kernels form the sums
    (SOLVERS)."""
    who = "value_and_grad"
    _solver(solver, who)
    X = _features(X, who)
    N, D = X.shape
    tg, wt, pr = _host_targets(targets, N, who), _host_weights(weights, N, who), _host_problems(problems, who)
    P = len(pr)
    W, b = torch.as_tensor(W), torch.as_tensor(b)
    if W.dim() != 3 or b.dim() != 2 or W.shape[0] != P or W.shape[2] != D or tuple(b.shape) != tuple(W.shape[:2]) or \
            not max(NUM_CLASSES[t] for t, _, _ in pr) <= W.shape[1] <= MAX_CLASSES:
        raise ValueError(f"{who}: W [{P}, n, {D}] and b [{P}, n] with n the classes of the widest label named, at most {MAX_CLASSES}")
    table, Cs = _tables(pr)
    ops.logreg_check_host(tg, wt, table, Cs, NUM_CLASSES)
    X = _require_gpu(X, who)
    dev, n = X.device, W.shape[1]
    Wd, bd = _pad_classes(W.to(dev, torch.float64)), _pad_classes(b.to(dev, torch.float64))
    F = torch.empty(P, dtype=torch.float64, device=dev)
    gW, gb = torch.empty_like(Wd), torch.empty_like(bd)
    if solver == "lockstep":
        cols = ops.logreg_columns(table[:, 2].tolist())
        ws = torch.empty(ops.logreg_lockstep_workspace(N, D, P, cols.numel(), False), dtype=torch.float64, device=dev)
        ops.logreg_value_grad_lockstep(X, tg.to(dev), wt.to(dev), table.to(dev), Cs.to(dev), cols.to(dev), Wd, bd, ws, F, gW, gb)
    else:
        ws = torch.empty(P * ops.logreg_workspace(N, D, False), dtype=torch.float64, device=dev)
        ops.logreg_value_grad(X, tg.to(dev), wt.to(dev), table.to(dev), Cs.to(dev), Wd, bd, ws, F, gW, gb)
    return F, gW[:, :n].contiguous(), gb[:, :n].contiguous()


# ---- the fit ------------------------------------------------------------------------------------------------------------------
class Fit:
    """What fit returns.  coef [P, n_max, D], intercept [P, n_max] float64 on the GPU (rows behind a label's classes are 0);
    problems [(label, C, weight row), ...] in launch order: weight row, then label, then C ascending as given; status [P] int32
    (STATUS names them), iterations [P] int32, objective, grad_norm [P] float64.  labels, Cs: what was swept; weights: the host
    rows [R, N] as given (before class_weight); n_classes [P]; solver: the one of SOLVERS that ran."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def index(self, label, C, row=0):
        """The position of problem (label, C, weight row)."""
        return self.problems.index((label, float(C), row))

    def ok(self):
        return self.status == 0


def default_chunk(N, D, P):
    return max(1, min(P, WORKSPACE_BYTES // (8 * ops.logreg_workspace(N, D, True))))


LAUNCH_WORK = 1 << 28  # N * D * iterations one launch may spend on a problem: a launch stays within seconds at the caps


def launch_iterations(N, D):
    """The L-BFGS iterations one launch runs at most (32 at small shapes, 4 at N = 16384, D = 4096)."""
    return max(1, min(32, LAUNCH_WORK // (N * D)))


def lockstep_chunk(N, D, P):
    """The problems of one lockstep chunk: as many as WORKSPACE_BYTES of workspace hold, every problem counted at 8 columns."""
    return max(1, min(P, WORKSPACE_BYTES // (8 * ops.logreg_lockstep_workspace(N, D, 1, MAX_CLASSES, True))))


def _launch_fits(X, tg, rows, launch, gtol, max_iter, chunk, who, launch_iters=None, solver="workgroup"):
    """The kernels' part of a fit: the host rows and launch problems are checked, uploaded and fitted `chunk` at a time, each
    chunk in launches of at most launch_iters iterations; between two launches the host reads the chunk's statuses."""
    _solver(solver, who)
    N, D = X.shape
    P = len(launch)
    if chunk is not None and (not resample.is_int(chunk) or chunk < 1):
        raise ValueError(f"{who}: chunk must be None or an integer >= 1, got {chunk!r}")
    table, Cd = _tables(launch)
    ops.logreg_check_host(tg, rows, table, Cd, NUM_CLASSES)
    X = _require_gpu(X, who)
    dev = X.device
    tg_d, rows_d, table_d, Cd_d = tg.to(dev), rows.to(dev), table.to(dev), Cd.to(dev)
    if launch_iters is not None and (not resample.is_int(launch_iters) or launch_iters < 1):
        raise ValueError(f"{who}: launch_iters must be None or an integer >= 1, got {launch_iters!r}")
    iters = launch_iterations(N, D) if launch_iters is None else launch_iters
    lockstep = solver == "lockstep"
    if lockstep:
        iters = min(iters, ops.LOGREG_LOCKSTEP_MAX_ITERS)
        c = min(lockstep_chunk(N, D, P) if chunk is None else chunk, P, ops.LOGREG_LOCKSTEP_MAX_PROBLEMS)
        ws = torch.empty(ops.logreg_lockstep_workspace(N, D, c, MAX_CLASSES * c, True), dtype=torch.float64, device=dev)
    else:
        c = default_chunk(N, D, P) if chunk is None else min(chunk, P)
        ws = torch.empty(c * ops.logreg_workspace(N, D, True), dtype=torch.float64, device=dev)
    coef = torch.empty(P, MAX_CLASSES, D, dtype=torch.float64, device=dev)
    intercept = torch.empty(P, MAX_CLASSES, dtype=torch.float64, device=dev)
    info = torch.empty(P, 2, dtype=torch.int32, device=dev)
    res = torch.empty(P, 2, dtype=torch.float64, device=dev)
    for p0 in range(0, P, c):
        p1 = min(P, p0 + c)
        resume = False
        cols = ops.logreg_columns(table[p0:p1, 2].tolist()).to(dev) if lockstep else None
        while True:
            if lockstep:
                ops.logreg_fit_lockstep(X, tg_d, rows_d, table_d[p0:p1], Cd_d[p0:p1], cols, gtol, max_iter, ws, coef[p0:p1],
                                        intercept[p0:p1], info[p0:p1], res[p0:p1], resume=resume, iters=iters)
            else:
                ops.logreg_fit(X, tg_d, rows_d, table_d[p0:p1], Cd_d[p0:p1], gtol, max_iter, ws, coef[p0:p1], intercept[p0:p1],
                               info[p0:p1], res[p0:p1], resume=resume, iters=iters)
            resume = True
            if not bool((info[p0:p1, 0] == ops.LOGREG_RUNNING).any()):  # the one readback between launches
                break
    return coef, intercept, info, res


def _as_fit(out, problems, labels, Cs, wt, class_weight, gtol, max_iter, solver):
    coef, intercept, info, res = out
    n_max = max(NUM_CLASSES[t] for t, _, _ in problems)
    return Fit(coef=coef[:, :n_max].contiguous(), intercept=intercept[:, :n_max].contiguous(), problems=problems,
               status=info[:, 0].contiguous(), iterations=info[:, 1].contiguous(), objective=res[:, 0].contiguous(),
               grad_norm=res[:, 1].contiguous(), labels=labels, Cs=Cs, weights=wt, class_weight=class_weight,
               n_classes=[NUM_CLASSES[t] for t, _, _ in problems], gtol=gtol, max_iter=max_iter, solver=solver)


def fit_problems(X, targets, problems, weights=None, gtol=1e-9, max_iter=1000, chunk=None, launch_iters=None, solver="workgroup"):
    """Fits the listed problems [(label, C, weight row), ...], in that order, over the one X [N, D] float32 on the GPU: what fit
    runs on, for a batch that is not a grid.  labels and Cs of the returned Fit are None."""
    who = "fit_problems"
    _solver(solver, who)
    X = _features(X, who)
    tg, wt, pr = _host_targets(targets, X.shape[0], who), _host_weights(weights, X.shape[0], who), _host_problems(problems, who)
    return _as_fit(_launch_fits(X, tg, wt, pr, gtol, max_iter, chunk, who, launch_iters, solver), pr, None, None, wt, None, gtol, max_iter,
                   solver)


def fit(X, targets, Cs=DEFAULT_CS, weights=None, class_weight=None, labels=range(8), gtol=1e-9, max_iter=1000, chunk=None,
        launch_iters=None, solver="workgroup"):
    """Fits every (weight row, label, C): P = R * len(labels) * len(Cs) problems over the one X [N, D] float32 on the GPU.  Stops a
    problem at |grad F|_inf <= gtol or after max_iter L-BFGS iterations.  class_weight: None or "balanced".  chunk: problems per
    launch (None: as many as WORKSPACE_BYTES of workspace hold), launch_iters: iterations per launch (None: launch_iterations(N,
    D)); the result depends on neither.  solver: one of SOLVERS."""
    who = "fit"
    _solver(solver, who)
    X = _features(X, who)
    N, D = X.shape
    tg, wt = _host_targets(targets, N, who), _host_weights(weights, N, who)
    labels, Cs = [int(t) for t in labels], [float(c) for c in Cs]
    if not labels or not Cs or len(set(labels)) != len(labels) or not all(0 <= t < len(NUM_CLASSES) for t in labels):
        raise ValueError(f"{who}: labels must be distinct labels in [0, {len(NUM_CLASSES)}) and Cs must not be empty")
    if class_weight not in (None, "none", "balanced"):
        raise ValueError(f"{who}: class_weight must be None or 'balanced', got {class_weight!r}")
    R = wt.shape[0]
    problems = [(t, c, r) for r in range(R) for t in labels for c in Cs]
    # the rows the kernels see: with "balanced" one per (weight row, label)
    if class_weight == "balanced":
        ops.logreg_check_host(tg, wt, *_tables(problems), NUM_CLASSES)  # before the class sums read the indices
        rows = torch.stack([balanced(wt, tg, t) for t in labels], dim=1).reshape(R * len(labels), N).contiguous()
        launch = [(t, c, r * len(labels) + labels.index(t)) for t, c, r in problems]
    else:
        rows, launch = wt, problems
    return _as_fit(_launch_fits(X, tg, rows, launch, gtol, max_iter, chunk, who, launch_iters, solver), problems, labels, Cs, wt,
                   class_weight, gtol, max_iter, solver)


# ---- prediction ---------------------------------------------------------------------------------------------------------------
def predict_all(fit, Xq, problems=None):
    """logits [len(problems), Q, n_max] float64 of the rows Xq [Q, D] under the problems (positions in fit.problems; None: all)."""
    who = "predict_logits"
    Xq = _require_gpu(_features(Xq, who, "Xq"), who)
    idx = list(range(len(fit.problems))) if problems is None else [int(p) for p in problems]
    if not idx or not all(0 <= p < len(fit.problems) for p in idx):
        raise ValueError(f"{who}: problems must be positions in [0, {len(fit.problems)})")
    if Xq.shape[1] != fit.coef.shape[2]:
        raise ValueError(f"{who}: Xq has {Xq.shape[1]} features, the fit {fit.coef.shape[2]}")
    dev, n_max = Xq.device, fit.coef.shape[1]
    sel = torch.tensor(idx, device=dev)
    coef, icpt = _pad_classes(fit.coef.to(dev)[sel]), _pad_classes(fit.intercept.to(dev)[sel])
    nts = torch.tensor([fit.n_classes[p] for p in idx], dtype=torch.int32, device=dev)
    out = torch.empty(len(idx), Xq.shape[0], MAX_CLASSES, dtype=torch.float64, device=dev)
    for p0 in range(0, len(idx), 65535):
        ops.logreg_predict(Xq, coef[p0:p0 + 65535], icpt[p0:p0 + 65535], nts[p0:p0 + 65535], out[p0:p0 + 65535])
    return out[:, :, :n_max]


def predict_logits(fit, Xq, which):
    """The list of 8 logit tensors [Q, n_t] float64 (the layout report.load_predictions returns) of the rows Xq under the 8
    problems `which`: one position in fit.problems per label, in label order."""
    which = [int(p) for p in which]
    if len(which) != len(NUM_CLASSES) or [fit.problems[p][0] for p in which] != list(range(len(NUM_CLASSES))):
        raise ValueError("predict_logits: `which` names one problem per label, in label order")
    z = predict_all(fit, Xq, which)
    return [z[t, :, :NUM_CLASSES[t]].contiguous() for t in range(len(NUM_CLASSES))]


# ---- weight rows --------------------------------------------------------------------------------------------------------------
def _order(N, seed, stream):
    """The cases in ascending order of their Philox word (word i of resample.philox_words(N, seed, 0, stream)), ties by index."""
    if not resample.is_int(seed) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"logreg: seed must be an integer in [0, 2^64), got {seed!r}")
    return np.argsort(resample.philox_words(N, seed, 0, stream), kind="stable")


def folds(N, K, seed):
    """[K, N] float64 0/1 rows: row k has 0 on the held-out cases of fold k and 1 elsewhere.  The case of rank j in the Philox
    order (stream 3) is held out in fold j % K: a partition, fold sizes within one of each other, a function of (N, K, seed)."""
    if not resample.is_int(N) or not resample.is_int(K) or not 2 <= K <= N:
        raise ValueError(f"folds: K must be an integer with 2 <= K <= N, got K = {K!r}, N = {N!r}")
    held = np.empty(N, dtype=np.int64)
    held[_order(N, seed, _FOLD_STREAM)] = np.arange(N) % K
    return torch.from_numpy((held[None, :] != np.arange(K)[:, None]).astype(np.float64))


def fractions(targets, fracs, seed):
    """[len(fracs), N] float64 0/1 rows, nested: the cases are put in the Philox order (stream 4); then, for every label and every
    class present in it, the first case of that class in the order is moved to the front (the anchors, at most 24, kept in their
    order).  Fraction f keeps the first max(ceil(f N), anchors) cases of that sequence -- so every class present in the full set
    is present in every fraction, and a smaller fraction's cases are among a larger one's."""
    t = torch.as_tensor(targets).cpu().numpy()
    N = t.shape[0]
    fracs = [float(f) for f in fracs]
    if not fracs or not all(0.0 < f <= 1.0 for f in fracs):
        raise ValueError(f"fractions: every fraction must lie in (0, 1], got {fracs!r}")
    order = _order(N, seed, _FRACTION_STREAM)
    anchors = set()
    for lab in range(t.shape[1]):
        seen = set()
        for i in order:
            if t[i, lab] not in seen:
                seen.add(t[i, lab])
                anchors.add(int(i))
    seq = [i for i in order if int(i) in anchors] + [i for i in order if int(i) not in anchors]
    rows = np.zeros((len(fracs), N))
    for r, f in enumerate(fracs):
        rows[r, seq[:max(int(math.ceil(f * N)), len(anchors))]] = 1.0
    return torch.from_numpy(rows)


# ---- selection ----------------------------------------------------------------------------------------------------------------
def score(logits, target, label, by):
    """The selection score of one label's logits [Q, n_t], larger is better: "auc" the AUROC of class CLS_WEIGHTS[label] (what
    AUC_AVG averages), "nll" minus the mean cross-entropy."""
    if by == "auc":
        return float(multiclass_auroc(logits, target, NUM_CLASSES[label])[CLS_WEIGHTS[label]])
    if by == "nll":
        return -float(torch.nn.functional.cross_entropy(logits.double(), target.long()))
    raise ValueError(f"select: by must be 'auc' or 'nll', got {by!r}")


def pick(table, Cs, per_label=True):
    """From the scores table [labels, len(Cs)] (larger is better): the C of each label's best column, or (per_label=False) the one
    C of the best column mean for all labels.  Ties take the smaller C."""
    table = np.asarray(table, dtype=np.float64)
    order = np.argsort(np.asarray(Cs, dtype=np.float64), kind="stable")  # ascending C: argmax takes the first of equals
    if not per_label:
        return [float(Cs[order[int(np.argmax(table.mean(axis=0)[order]))]])] * table.shape[0]
    return [float(Cs[order[int(np.argmax(row[order]))]]) for row in table]


def select(fit, Xval=None, tval=None, by="auc", per_label=True, X=None, targets=None):
    """Picks C.  With (Xval, tval): every problem of weight row 0 is scored on the validation rows.  With Xval = None and the
    training (X, targets): every case is scored by the problem of the one weight row that holds it out (its weight there is 0 --
    the rows of `folds`), the out-of-fold predictions pooled over the folds.  Returns {"C": [per label of fit.labels], "table":
    [labels, Cs] scores (larger is better; "nll" scores are minus the NLL), "Cs", "labels", "by"}."""
    if by not in ("auc", "nll"):
        raise ValueError(f"select: by must be 'auc' or 'nll', got {by!r}")
    R, nl, nc = fit.weights.shape[0], len(fit.labels), len(fit.Cs)
    table = np.zeros((nl, nc))
    if Xval is not None:
        z = predict_all(fit, Xval, range(nl * nc))  # weight row 0
        tv = torch.as_tensor(tval).to(z.device)
        for a, t in enumerate(fit.labels):
            for j in range(nc):
                table[a, j] = score(z[a * nc + j, :, :NUM_CLASSES[t]], tv[:, t], t, by)
    else:
        if X is None or targets is None:
            raise ValueError("select: validation rows (Xval, tval), or the training (X, targets) of a fit on folds")
        held = fit.weights == 0
        if R < 2 or not bool((held.sum(dim=0) == 1).all()):
            raise ValueError("select: out-of-fold selection needs weight rows that hold every case out exactly once (folds)")
        z = predict_all(fit, X)
        z = z.reshape(R, nl, nc, *z.shape[1:])
        tv = torch.as_tensor(targets).to(z.device)
        owner = held.double().argmax(dim=0).to(z.device)  # the row that holds case i out
        cases = torch.arange(X.shape[0], device=z.device)
        for a, t in enumerate(fit.labels):
            for j in range(nc):
                zz = z[owner, a, j, cases]
                table[a, j] = score(zz[:, :NUM_CLASSES[t]], tv[:, t], t, by)
    return {"C": pick(table, fit.Cs, per_label), "table": torch.from_numpy(table), "Cs": list(fit.Cs), "labels": list(fit.labels),
            "by": by}


# ---- normalisation ------------------------------------------------------------------------------------------------------------
def normalize_fit(X, kind):
    """The normalisation `kind` of the features X [N, D] float32: "none", "l2" (rows to unit norm, as knn.normalize) or
    "standardize" (per-feature mean and standard deviation over ALL N rows in fp64, a feature of deviation 0 is only centred).
    The scaling does not depend on the weight rows: under K-fold selection the features of the held-out cases -- never their
    labels -- enter the mean and the deviation.  That is intended: the scaling is part of the frozen feature map, the same for
    every problem, so that all problems share one X."""
    if kind not in NORMALIZE:
        raise ValueError(f"normalize_fit: kind must be one of {NORMALIZE}, got {kind!r}")
    X = _features(X, "normalize_fit")
    norm = {"kind": kind}
    if kind == "standardize":
        x = X.double()
        std = x.std(dim=0, unbiased=False)
        norm.update(mean=x.mean(dim=0), std=torch.where(std > 0, std, torch.ones_like(std)))
    return norm


def normalize_apply(X, norm):
    """float32 features under normalize_fit's `norm`: standardize = float32((x - mean) / std) from fp64."""
    X = _features(X, "normalize_apply", "Xq")
    if norm["kind"] == "none":
        return X.contiguous()
    if norm["kind"] == "l2":
        from .knn import normalize
        return normalize(X)
    return ((X.double() - norm["mean"].to(X.device)) / norm["std"].to(X.device)).float().contiguous()


def to_baseline_state(fit, which, norm):
    """{"classifier.{t}.weight" [n_t, D], "classifier.{t}.bias" [n_t]} float32 for a Baseline state_dict from the 8 problems
    `which` (as predict_logits).  "standardize" is folded in: W' = W / std, b' = b - W' . mean, so the heads take the raw
    features.  "l2" scales each row by its own norm, which no affine map does: it raises.  A class without weight keeps its
    intercept -inf (its logit is -inf, its probability 0) as a float32 bias.  The explanation methods run on such heads with
    target="pred" (the class is never the argmax; tests/test_logreg_gpu.py); a target that names that class is not meaningful."""
    if norm["kind"] == "l2":
        raise ValueError("to_baseline_state: l2 normalisation divides each row by its own norm; it cannot be folded into Linear "
                         "heads -- fit with 'standardize' or 'none' to export heads")
    which = [int(p) for p in which]
    if len(which) != len(NUM_CLASSES) or [fit.problems[p][0] for p in which] != list(range(len(NUM_CLASSES))):
        raise ValueError("to_baseline_state: `which` names one problem per label, in label order")
    state = {}
    for t, p in enumerate(which):
        W, b = fit.coef[p, :NUM_CLASSES[t]].double(), fit.intercept[p, :NUM_CLASSES[t]].double()
        if norm["kind"] == "standardize":
            W = W / norm["std"].to(W.device)
            b = b - W @ norm["mean"].to(W.device)
        state[f"classifier.{t}.weight"] = W.float().cpu().contiguous()
        state[f"classifier.{t}.bias"] = b.float().cpu().contiguous()
    return state
