"""Times sm3hip.logreg.fit() over the default grid (8 labels x 16 values of C log-spaced over 1e-4 .. 1e4 = 128 problems) against a
scikit-learn loop (LogisticRegression(solver="lbfgs", tol=1e-10, max_iter=10000) per label and C on the host cores the job may
use) on the same standardised features, at N = 413, D = 4096 (the derm7pt train split under the ResNet-50 encoders) and N = 8192,
D = 4096.

    python tools/logreg_bench.py --out profiles/logreg_measure.json
    python tools/logreg_bench.py --only fit --solver both --out profiles/logreg_lockstep_measure.json
    rocprofv3 --kernel-trace --stats --output-format csv -d out -o logreg -- python tools/logreg_bench.py --only fit --sizes 413

fit() is timed end to end -- the host checks, the uploads, every launch, by the host clock around a final device synchronise --
after a warm-up call on the same shape (two C values); --repeats times, the median is reported beside every value.  "launch_s" is
the time between two device events around the same call: the kernels' time, the host work before the first launch left out.
scikit-learn runs once per (label, C); --sklearn-cs limits its loop to some of the grid's values (at N = 8192 the whole loop takes
longer than a job may), and the record says which were run and sums only those.  Per C the worst gap between the two sides'
probabilities on --queries held-out rows is recorded, and per problem the status and the iterations of fit().  Kernel time per
kernel comes from a separate run under rocprofv3 --kernel-trace --stats with --only fit (tracing slows the host)."""
import argparse
import json
import os
import statistics
import sys
import time

SCRIPT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_PATH = os.path.split(SCRIPT_DIR)[0]
sys.path.insert(0, ROOT_PATH)

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: see sm3hip/__init__.py

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sm3hip import logreg  # noqa: E402
from sm3hip.metrics import NUM_CLASSES  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser(description="logreg.fit() against a scikit-learn loop (MI355X)")
    p.add_argument("--sizes", type=int, nargs="*", default=[413, 8192], help="train rows")
    p.add_argument("--dim", type=int, default=4096)
    p.add_argument("--queries", type=int, default=256, help="held-out rows the probabilities are compared on")
    p.add_argument("--cs", type=float, nargs="*", default=list(logreg.DEFAULT_CS))
    p.add_argument("--sklearn-cs", type=float, nargs="*", default=None,
                   help="the values of --cs the scikit-learn loop runs (default: all)")
    p.add_argument("--gtol", type=float, default=1e-9)
    p.add_argument("--max-iter", type=int, default=1000)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--only", choices=("both", "fit", "sklearn"), default="both")
    p.add_argument("--solver", choices=logreg.SOLVERS + ("both",), default="workgroup",
                   help="the solver timed; both: the two alternate in one process, run by run, and the record holds each "
                        "(the lockstep solver's figures under lockstep_*)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", type=str, default=None, help="JSON file of the result records")
    p.add_argument("--append", action="store_true", help="keep the records --out already holds and add this run's")
    return p


def make_inputs(N, Q, D, seed):
    """(X [N, D], targets [N, 8], Xq [Q, D]) on the CPU from a CPU generator: standard normal features standardised over the N
    rows, each label the argmax of a random linear map of 64 of the features plus noise -- learnable, not noise-free."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N + Q, D, generator=g)
    t = []
    for n in NUM_CLASSES:
        a = torch.randn(64, n, generator=g) / 8.0
        t.append((x[:, :64] @ a + 0.7 * torch.randn(N + Q, n, generator=g)).argmax(dim=1))
    norm = logreg.normalize_fit(x[:N].contiguous(), "standardize")
    xs = logreg.normalize_apply(x, norm)
    return xs[:N].contiguous(), torch.stack(t, dim=1)[:N].contiguous(), xs[N:].contiguous()


def time_fit(X, T, Cs, args, solver="workgroup"):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    f = logreg.fit(X, T, Cs, gtol=args.gtol, max_iter=args.max_iter, solver=solver)
    end.record()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, start.elapsed_time(end) / 1e3, f


def sklearn_loop(X, T, Xq, Cs):
    """{(label, C): probabilities [Q, n_t]} and the seconds of each fit."""
    from sklearn.linear_model import LogisticRegression
    x, xq = X.double().numpy(), Xq.double().numpy()
    out, secs, iters = {}, {}, {}
    for t, n in enumerate(NUM_CLASSES):
        y = T[:, t].numpy()
        for c in Cs:
            m = LogisticRegression(C=2.0 * c if len(np.unique(y)) == 2 else c, solver="lbfgs", tol=1e-10, max_iter=10000)
            t0 = time.perf_counter()
            m.fit(x, y)
            secs[(t, c)] = time.perf_counter() - t0
            pr = np.zeros((xq.shape[0], n))
            pr[:, m.classes_] = m.predict_proba(xq)
            out[(t, c)], iters[(t, c)] = pr, int(np.max(m.n_iter_))
        print(f"scikit-learn: label {t} done, {sum(secs.values()):.1f} s so far", file=sys.stderr, flush=True)
    return out, secs, iters


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not torch.cuda.is_available() and args.only != "sklearn":
        raise SystemExit("logreg_bench: needs a GPU")
    Cs = sorted(float(c) for c in args.cs)
    sk_cs = Cs if args.sklearn_cs is None else sorted(float(c) for c in args.sklearn_cs)
    if not set(sk_cs) <= set(Cs):
        raise SystemExit("logreg_bench: --sklearn-cs must be among --cs")
    records = []
    for N in args.sizes:
        X, T, Xq = make_inputs(N, args.queries, args.dim, args.seed)
        rec = {"N": N, "D": args.dim, "Cs": Cs, "problems": len(Cs) * len(NUM_CLASSES), "gtol": args.gtol, "max_iter": args.max_iter}
        fit = None
        if args.only != "sklearn":
            Xd = X.cuda()
            solvers = logreg.SOLVERS if args.solver == "both" else (args.solver,)
            for s in solvers:
                time_fit(Xd, T, Cs[len(Cs) // 2:len(Cs) // 2 + 2], args, s)  # warm-up on this shape: code objects, the allocator
            walls, launches, fits = {s: [] for s in solvers}, {s: [] for s in solvers}, {}
            for _ in range(args.repeats):
                for s in solvers:  # the solvers alternate, so that a drift of the machine meets both
                    w, l, fits[s] = time_fit(Xd, T, Cs, args, s)
                    walls[s].append(w)
                    launches[s].append(l)
            for s in solvers:
                # with --solver both the workgroup solver keeps the record's plain keys, the lockstep solver's carry its name
                pre = "lockstep_" if s == "lockstep" and len(solvers) > 1 else ""
                status = fits[s].status.cpu().numpy()
                rec.update({pre + "fit_s": statistics.median(walls[s]), pre + "fit_s_all": walls[s],
                            pre + "launch_s": statistics.median(launches[s]), pre + "launch_s_all": launches[s],
                            pre + "iterations": int(fits[s].iterations.sum()), pre + "iterations_max": int(fits[s].iterations.max()),
                            pre + "status_counts": {logreg.STATUS[k]: int((status == k).sum()) for k in range(len(logreg.STATUS))},
                            pre + "grad_norm_max": float(fits[s].grad_norm.max())})
            rec.update(solver=args.solver, device=torch.cuda.get_device_name(0))
            fit = fits[solvers[0]]
            if len(solvers) > 1:  # the two optima on the held-out rows: the worst probability gap between the solvers
                za, zb = (logreg.predict_all(fits[s], Xq.cuda()) for s in solvers)
                gap = 0.0
                for p, n in enumerate(fit.n_classes):
                    gap = max(gap, float((torch.softmax(za[p, :, :n], dim=1) - torch.softmax(zb[p, :, :n], dim=1)).abs().max()))
                rec["solver_probability_gap"] = gap
        if args.only != "fit":
            import sklearn
            probs, secs, iters = sklearn_loop(X, T, Xq, sk_cs)
            rec.update(sklearn_cs=sk_cs, sklearn_s=sum(secs.values()), sklearn_s_per_c={repr(c): sum(s for (t, cc), s in secs.items() if cc == c)
                                                                                        for c in sk_cs},
                       sklearn_iterations_max=max(iters.values()), sklearn=sklearn.__version__, cpu_threads=torch.get_num_threads())
            if fit is not None:
                z = logreg.predict_all(fit, Xq.cuda())
                gap = {}
                for c in sk_cs:
                    worst = 0.0
                    for t, n in enumerate(NUM_CLASSES):
                        pr = torch.softmax(z[fit.index(t, c), :, :n], dim=1).cpu().numpy()
                        worst = max(worst, float(np.abs(pr - probs[(t, c)]).max()))
                    gap[repr(c)] = worst
                rec["probability_gap_per_c"] = gap
                if len(sk_cs) == len(Cs):
                    rec["ratio"] = rec["sklearn_s"] / rec["fit_s"]
        records.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        if args.append and os.path.isfile(args.out):
            records = json.load(open(args.out))["records"] + records
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/logreg_bench.py", "records": records}, f, indent=1)
            f.write("\n")
    return records


if __name__ == "__main__":
    main()
