"""Times sm3hip.conformal.conformal_report(bootstrap=B) against the numpy loop a user could write without it: per replicate,
draw both resamples, re-sort the resampled true-class calibration scores of every label (of every class in class mode), take
the order statistic per level, and count the sets of the resampled test split -- at N_cal = N = 395 (derm7pt's splits) and at
MAX_CASES, for both scores and both conditionings.  The loop starts from the same int64 score tables as the kernel (the
softmax and the fixed-point step are outside its timing).

    python tools/conformal_bench.py --bootstrap 2000 --loop-replicates 20 --out profiles/conformal_measure.json

The report is timed whole (scores, the sort, launches, the copy back and the host's values and order statistics), between
device synchronisations: the median and the range of --repeats calls after a warm-up call; the launches alone are timed with
device events.  The loop is timed over --loop-replicates replicates after a warm-up and scaled to B (every replicate costs the
same).  Kernel time comes from a separate run under rocprofv3 --kernel-trace --stats with --only report."""
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

from sm3hip import conformal, metrics, ops, report  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser(description="conformal_report(bootstrap=B) against a numpy resampling loop (MI355X)")
    p.add_argument("--bootstrap", type=int, default=2000)
    p.add_argument("--sizes", type=int, nargs="*", default=[395, report.MAX_CASES])
    p.add_argument("--methods", nargs="*", choices=conformal.METHODS, default=list(conformal.METHODS))
    p.add_argument("--conditionals", nargs="*", choices=conformal.CONDITIONALS, default=list(conformal.CONDITIONALS))
    p.add_argument("--alphas", type=float, nargs="*", default=list(conformal.DEFAULT_ALPHAS))
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--loop-replicates", type=int, default=20)
    p.add_argument("--only", choices=("both", "report", "loop"), default="both")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", type=str, default=None, help="JSON file of the result records")
    return p


def make_inputs(N, seed, dev):
    """Seeded logits (twice a standard normal: a moderately confident classifier) and labels."""
    g = torch.Generator().manual_seed(seed)
    targets = torch.stack([torch.randint(0, n, (N,), generator=g) for n in metrics.NUM_CLASSES], dim=1)
    preds = [2.0 * torch.randn(N, n, generator=g) for n in metrics.NUM_CLASSES]
    return [p.to(dev) for p in preds], targets.to(dev)


def time_report(test, cal, B, alphas, method, conditional, seed, repeats):
    kw = dict(alphas=alphas, method=method, conditional=conditional, bootstrap=B, seed=seed)
    conformal.conformal_report(*test, *cal, **kw)  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        conformal.conformal_report(*test, *cal, **kw)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    # the launches alone, by device events
    dev = test[1].device
    inp = conformal._device_inputs(*test, *cal, [1.0] * conformal.T, method, dev)
    levels = conformal.check_alphas(alphas)[1]
    counts = torch.empty((B, conformal.T, len(levels), conformal.RECORD), dtype=torch.int64, device=dev)
    thr = torch.empty((B, conformal.T, len(levels), conformal.MAX_CLASSES), dtype=torch.int64, device=dev)
    c = conformal.DEFAULT_CHUNK
    kern = []
    for _ in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for r0 in range(0, B, c):
            e = r0 + min(c, B - r0)
            ops.conformal_counts(*inp, levels, counts[r0:e], thr[r0:e], conditional, seed, r0)
        b.record()
        torch.cuda.synchronize()
        kern.append(a.elapsed_time(b) / 1e3)
    return statistics.median(times), min(times), max(times), statistics.median(kern[1:])


def loop_replicate(s, y, cal_a, cal_y, levels, conditional, rng):
    """What a user writes in numpy alone, from the score tables: both resamples, the re-sorted calibration scores, the order
    statistic per label / level (/ class), the set counts of the resampled test split."""
    N, N_cal = y.shape[0], cal_y.shape[0]
    ic, it = rng.integers(0, N_cal, N_cal), rng.integers(0, N, N)
    out = []
    for t, n in enumerate(metrics.NUM_CLASSES):
        k0 = report.COLUMN_PAIRS.index((t, 0))
        a, yc = cal_a[t, ic], cal_y[ic, t]
        st, yt = s[k0:k0 + n][:, it], y[it, t]
        groups = [np.sort(a)] if conditional == "marginal" else [np.sort(a[yc == c]) for c in range(n)]
        for num, den in levels:
            thr = np.empty(n, dtype=np.int64)
            for c in range(n):
                g = groups[0] if conditional == "marginal" else groups[c]
                k = (len(g) + 1) - ((len(g) + 1) * num) // den
                thr[c] = conformal.INF if k > len(g) else g[k - 1]
            inset = st <= thr[:, None]
            size = inset.sum(axis=0)
            hit = yt[None, :] == np.arange(n)[:, None]
            covered = (inset & hit).any(axis=0)
            out.append([covered.sum(), size.sum(), (covered & (size == 1)).sum(), *np.bincount(size, minlength=6),
                        *hit.sum(axis=1), *(inset & hit).sum(axis=1), *inset.sum(axis=1)])
    return out


def time_loop(test, cal, alphas, method, conditional, replicates, seed):
    s, cal_s = (conformal.scores(p, None, method) for p in (test[0], cal[0]))
    cal_a = conformal.true_class_scores(cal_s, cal[1]).cpu().numpy()
    s, y, cal_y = s.cpu().numpy(), test[1].cpu().numpy(), cal[1].cpu().numpy()
    levels = conformal.check_alphas(alphas)[1]
    rng = np.random.default_rng(seed)
    for _ in range(2):
        loop_replicate(s, y, cal_a, cal_y, levels, conditional, rng)
    t0 = time.perf_counter()
    for _ in range(replicates):
        loop_replicate(s, y, cal_a, cal_y, levels, conditional, rng)
    return (time.perf_counter() - t0) / replicates


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("conformal_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    records = []
    for N in args.sizes:
        test, cal = make_inputs(N, args.seed + N, dev), make_inputs(N, args.seed + N + 1, dev)
        for method in args.methods:
            for conditional in args.conditionals:
                rec = {"N": N, "N_cal": N, "bootstrap": args.bootstrap, "alphas": args.alphas, "method": method,
                       "conditional": conditional}
                if args.only in ("both", "report"):
                    med, lo, hi, kern = time_report(test, cal, args.bootstrap, args.alphas, method, conditional, args.seed,
                                                    args.repeats)
                    rec.update({"report_s": med, "report_s_min": lo, "report_s_max": hi, "report_launches_s": kern,
                                "repeats": args.repeats})
                if args.only in ("both", "loop"):
                    per = time_loop(test, cal, args.alphas, method, conditional, args.loop_replicates, args.seed)
                    rec.update({"loop_s_per_replicate": per, "loop_s_scaled": per * args.bootstrap,
                                "loop_replicates_timed": args.loop_replicates})
                if "report_s" in rec and "loop_s_scaled" in rec:
                    rec["loop_over_report"] = rec["loop_s_scaled"] / rec["report_s"]
                print(json.dumps(rec), flush=True)
                records.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
    return records


if __name__ == "__main__":
    main()
