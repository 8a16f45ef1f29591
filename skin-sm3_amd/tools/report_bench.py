"""Times sm3hip.report.evaluation_report(bootstrap=B) against the loop a user could write without it: per replicate, resample
the rows on the GPU and call metrics.multiclass_auroc per label (24 one-vs-rest AUROCs: an argsort and two host reads each) --
at N = 395 (derm7pt's test split) and at N = MAX_CASES.  The loop gives the AUROC only; the report also gives Recall, Spec and
Prec from the same launch.

    python tools/report_bench.py --bootstrap 2000 --loop-replicates 40 --out profiles/report_measure.json

The report is timed whole (ranking, launches, the copy back and the host's values, averages and order statistics), between
device synchronisations, the median of --repeats calls after a warm-up call; the launches alone are timed with device events.
The loop is timed over --loop-replicates replicates after a warm-up and scaled to B (every replicate costs the same).  Both
sides see the same seeded predictions with tied scores.  Kernel time comes from a separate run under
rocprofv3 --kernel-trace --stats with --only report."""
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

import torch  # noqa: E402

from sm3hip import metrics, ops, report  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser(description="evaluation_report(bootstrap=B) against a torch resampling loop (MI355X)")
    p.add_argument("--bootstrap", type=int, default=2000)
    p.add_argument("--sizes", type=int, nargs="*", default=[395, report.MAX_CASES])
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--loop-replicates", type=int, default=40)
    p.add_argument("--only", choices=("both", "report", "loop"), default="both")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", type=str, default=None, help="JSON file of the result records")
    return p


def make_inputs(N, seed, dev):
    """Seeded logits in steps of 1/4 (tied scores, as a saturated classifier gives) and labels."""
    g = torch.Generator().manual_seed(seed)
    targets = torch.stack([torch.randint(0, n, (N,), generator=g) for n in metrics.NUM_CLASSES], dim=1)
    preds = [(4.0 * torch.randn(N, n, generator=g)).round() / 4.0 for n in metrics.NUM_CLASSES]
    return [p.to(dev) for p in preds], targets.to(dev)


def time_report(preds, targets, B, seed, repeats):
    report.evaluation_report(preds, targets, bootstrap=B, seed=seed)  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        report.evaluation_report(preds, targets, bootstrap=B, seed=seed)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    # the launches alone, by device events
    dev = targets.device
    order, gs, ge, yhat = report.ranking(preds, targets)
    y = targets.int().contiguous()
    colmap = torch.tensor(report.COLUMN_PAIRS, dtype=torch.int32, device=dev)
    out = torch.empty((B, report.K, 6), dtype=torch.int64, device=dev)
    kern = []
    for _ in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for r0 in range(0, B, report.DEFAULT_CHUNK):
            ops.report_counts(order, gs, ge, y, yhat, colmap, out[r0:r0 + min(report.DEFAULT_CHUNK, B - r0)], seed, r0)
        b.record()
        torch.cuda.synchronize()
        kern.append(a.elapsed_time(b) / 1e3)
    return statistics.median(times), min(times), max(times), statistics.median(kern[1:])


def loop_replicate(preds, targets, gen):
    """What a user writes on metrics.py alone: resample the rows, 24 AUROCs."""
    N = targets.shape[0]
    idx = torch.randint(0, N, (N,), device=targets.device, generator=gen)
    t = targets[idx]
    return [metrics.multiclass_auroc(p[idx], t[:, i], n) for i, (p, n) in enumerate(zip(preds, metrics.NUM_CLASSES))]


def time_loop(preds, targets, replicates, seed):
    gen = torch.Generator(device=targets.device).manual_seed(seed)
    for _ in range(2):
        loop_replicate(preds, targets, gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replicates):
        loop_replicate(preds, targets, gen)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / replicates


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("report_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    records = []
    for N in args.sizes:
        preds, targets = make_inputs(N, args.seed + N, dev)
        rec = {"N": N, "bootstrap": args.bootstrap}
        if args.only in ("both", "report"):
            med, lo, hi, kern = time_report(preds, targets, args.bootstrap, args.seed, args.repeats)
            rec.update({"report_s": med, "report_s_min": lo, "report_s_max": hi, "report_launches_s": kern,
                        "repeats": args.repeats})
        if args.only in ("both", "loop"):
            per = time_loop(preds, targets, args.loop_replicates, args.seed)
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
