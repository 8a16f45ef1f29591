"""Times sm3hip.calibration.calibration_report(bootstrap=B) against the loop a user could write without it: per replicate,
resample the rows on the GPU with torch.randint and, per label, softmax, NLL, Brier and a bucketize / scatter-add ECE of the top
label and of every class column (32 series) -- at N = 395 (derm7pt's test split) and at N = MAX_CASES, for both binnings (the
loop's mass binning is the quantile form: it sorts the resampled scores of every series in every replicate).

    python tools/calib_bench.py --bootstrap 2000 --loop-replicates 40 --out profiles/calib_measure.json

The report is timed whole (fixed-point series, the sort, launches, the copy back and the host's values and order statistics),
between device synchronisations, the median of --repeats calls after a warm-up call; the launches alone are timed with device
events.  The loop is timed over --loop-replicates replicates after a warm-up and scaled to B (every replicate costs the same).
Both sides see the same seeded predictions.  Kernel time comes from a separate run under rocprofv3 --kernel-trace --stats with
--only report."""
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

from sm3hip import calibration, metrics, ops, report  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser(description="calibration_report(bootstrap=B) against a torch resampling loop (MI355X)")
    p.add_argument("--bootstrap", type=int, default=2000)
    p.add_argument("--sizes", type=int, nargs="*", default=[395, report.MAX_CASES])
    p.add_argument("--binnings", nargs="*", choices=calibration.BINNINGS, default=list(calibration.BINNINGS))
    p.add_argument("--bins", type=int, default=calibration.DEFAULT_BINS)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--loop-replicates", type=int, default=40)
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


def time_report(preds, targets, B, M, binning, seed, repeats):
    kw = dict(bins=M, binning=binning, bootstrap=B, seed=seed)
    calibration.calibration_report(preds, targets, **kw)  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        calibration.calibration_report(preds, targets, **kw)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    # the launches alone, by device events
    dev = targets.device
    q, ev, xq = calibration.fixed_point(preds, targets)
    order = torch.sort(q, dim=1, stable=True).indices.int().contiguous()
    slabel = torch.tensor(calibration.SERIES_LABEL, dtype=torch.int32, device=dev)
    bins = torch.empty((B, calibration.S, M, 3), dtype=torch.int64, device=dev)
    sums = torch.empty((B, calibration.X), dtype=torch.int64, device=dev)
    c = calibration.DEFAULT_CHUNK
    kern = []
    for _ in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for r0 in range(0, B, c):
            e = r0 + min(c, B - r0)
            ops.calib_counts(q, ev, order, slabel, xq, bins[r0:e], sums[r0:e], calibration.T, binning, seed, r0)
        b.record()
        torch.cuda.synchronize()
        kern.append(a.elapsed_time(b) / 1e3)
    return statistics.median(times), min(times), max(times), statistics.median(kern[1:])


def _ece(conf, hit, M, binning):
    """ECE of one series in torch: bucketize, scatter-add, sum of |acc - conf| weighted by the bin's share."""
    N = conf.shape[0]
    if binning == "width":
        b = torch.clamp((conf * M).long(), max=M - 1)
    else:
        b = torch.empty_like(conf, dtype=torch.long)
        b[torch.argsort(conf, stable=True)] = (torch.arange(N, device=conf.device) * M) // N
    n = torch.zeros(M, dtype=torch.float64, device=conf.device).scatter_add_(0, b, torch.ones_like(conf))
    e = torch.zeros_like(n).scatter_add_(0, b, hit.double())
    s = torch.zeros_like(n).scatter_add_(0, b, conf)
    return (e - s).abs().sum() / N


def loop_replicate(preds, targets, M, binning, gen):
    """What a user writes in torch alone: resample the rows; per label NLL, Brier, top-label ECE and the class-wise ECEs."""
    N = targets.shape[0]
    idx = torch.randint(0, N, (N,), device=targets.device, generator=gen)
    out = []
    for t, pr in enumerate(preds):
        z, y = pr[idx].double(), targets[idx, t]
        p, lp = torch.softmax(z, 1), torch.log_softmax(z, 1)
        onehot = torch.nn.functional.one_hot(y, p.shape[1]).double()
        out.append(-lp.gather(1, y[:, None]).mean())
        out.append(((p - onehot) ** 2).sum(1).mean())
        conf, yhat = p.max(dim=1)
        out.append(_ece(conf, yhat == y, M, binning))
        for c in range(p.shape[1]):
            out.append(_ece(p[:, c].contiguous(), y == c, M, binning))
    return torch.stack(out)


def time_loop(preds, targets, M, binning, replicates, seed):
    gen = torch.Generator(device=targets.device).manual_seed(seed)
    for _ in range(2):
        loop_replicate(preds, targets, M, binning, gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replicates):
        loop_replicate(preds, targets, M, binning, gen)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / replicates


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("calib_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    records = []
    for N in args.sizes:
        preds, targets = make_inputs(N, args.seed + N, dev)
        for binning in args.binnings:
            rec = {"N": N, "bootstrap": args.bootstrap, "bins": args.bins, "binning": binning}
            if args.only in ("both", "report"):
                med, lo, hi, kern = time_report(preds, targets, args.bootstrap, args.bins, binning, args.seed, args.repeats)
                rec.update({"report_s": med, "report_s_min": lo, "report_s_max": hi, "report_launches_s": kern,
                            "repeats": args.repeats})
            if args.only in ("both", "loop"):
                per = time_loop(preds, targets, args.bins, binning, args.loop_replicates, args.seed)
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
