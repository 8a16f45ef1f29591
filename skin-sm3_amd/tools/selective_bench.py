"""Times sm3hip.selective.selective_report(bootstrap=B) against the loop a user could write with numpy: per replicate and label
resample the cases, sort them stably by confidence, take cumulative sums of the errors and of the 2 x 2 events, then the area
under the risk-coverage curve, the values at the coverage cuts and the largest cut within each risk level -- at N = 395
(derm7pt's test split) and at N = MAX_CASES.

    python tools/selective_bench.py --bootstrap 2000 --loop-replicates 20 --out profiles/selective_measure.json

The report is timed whole (keys, ranking, launches, the copy back and the host's values and order statistics), between device
synchronisations, the median of --repeats calls after a warm-up call; the launches alone are timed with device events.  Beside
them, with the same events, N and B, the launches of sm3_report_counts (evaluation_report's kernel): the yardstick for "one more
kernel of the same family".  The loop is timed over --loop-replicates replicates after a warm-up and scaled to B (every replicate
costs the same); it is fed the multiplicities of the report's own replicates (Philox4x32-10 restated in numpy,
tools/operating_bench.py), and the AURC of its first replicate is held against the report's as a check that both sides compute
the same thing."""
import argparse
import json
import os
import statistics
import sys
import time

SCRIPT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_PATH = os.path.split(SCRIPT_DIR)[0]
sys.path.insert(0, ROOT_PATH)
sys.path.insert(0, SCRIPT_DIR)

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: see sm3hip/__init__.py

import numpy as np  # noqa: E402
import torch  # noqa: E402

from operating_bench import make_inputs, multiplicities  # noqa: E402
from sm3hip import ops, report, selective  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser(description="selective_report(bootstrap=B) against a numpy resampling loop (MI355X)")
    p.add_argument("--bootstrap", type=int, default=2000)
    p.add_argument("--sizes", type=int, nargs="*", default=[395, report.MAX_CASES])
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--loop-replicates", type=int, default=20)
    p.add_argument("--only", choices=("both", "report", "loop"), default="both")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", type=str, default=None, help="JSON file of the result records")
    return p


def _events(fn, repeats):
    """Median device time in seconds of fn() over `repeats` calls after one warm-up call."""
    t = []
    for _ in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) / 1e3)
    return statistics.median(t[1:])


def time_report(preds, targets, B, seed, repeats):
    selective.selective_report(preds, targets, bootstrap=B, seed=seed)  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        selective.selective_report(preds, targets, bootstrap=B, seed=seed)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dev, N = targets.device, targets.shape[0]
    key = selective.keys(preds, "msp")
    order, last, _, _ = selective.ranking(key, key)
    packed = selective.pack_flags(preds, targets, order, last)
    table = torch.from_numpy(selective.harmonic_table(N)).to(dev)
    cov, risks = selective.check_coverages(selective.DEFAULT_COVERAGES)[1], selective.check_risks(selective.DEFAULT_RISKS)[1]
    kc = torch.tensor(selective.coverage_cuts(N, cov), dtype=torch.int32, device=dev)
    pc = torch.zeros((8, 0), dtype=torch.int32, device=dev)
    rk = torch.tensor(risks, dtype=torch.int32, device=dev)
    out = torch.empty((B, 8, ops.selective_record(len(cov), len(risks), 0)), dtype=torch.int64, device=dev)

    def launches():
        for r0 in range(0, B, selective.DEFAULT_CHUNK):
            ops.selective_counts(packed, order, table, kc, pc, rk, out[r0:r0 + min(selective.DEFAULT_CHUNK, B - r0)], seed, r0)
    whole = _events(launches, repeats)
    point = _events(lambda: ops.selective_counts(packed, order, table, kc, pc, rk, out[:1], seed, 0, point=True), repeats)
    # the yardstick: evaluation_report's kernel at the same N and B
    o24, g24s, g24e, yhat = report.ranking(preds, targets)
    y = targets.int().contiguous()
    colmap = torch.tensor(report.COLUMN_PAIRS, dtype=torch.int32, device=dev)
    rout = torch.empty((B, report.K, 6), dtype=torch.int64, device=dev)

    def report_launches():
        for r0 in range(0, B, report.DEFAULT_CHUNK):
            ops.report_counts(o24, g24s, g24e, y, yhat, colmap, rout[r0:r0 + min(report.DEFAULT_CHUNK, B - r0)], seed, r0)
    yard = _events(report_launches, repeats)
    return {"report_s": statistics.median(times), "report_s_min": min(times), "report_s_max": max(times),
            "selective_launches_s": whole, "launch_share": whole / statistics.median(times), "selective_point_launch_s": point,
            "report_counts_launches_s": yard, "selective_over_report_counts": whole / yard, "repeats": repeats}


def loop_replicate(key, err, pos, call, m, kcuts, risks):
    """What a user writes on numpy for one replicate; returns the AURC of the 8 labels."""
    idx = np.repeat(np.arange(m.shape[0]), m)                       # the resampled cases
    n = idx.shape[0]
    k = np.arange(1, n + 1)
    aurc = np.zeros(key.shape[0])
    for t in range(key.shape[0]):
        o = idx[np.argsort(-key[t][idx], kind="stable")]
        ks = key[t][o]
        e = np.cumsum(err[t][o])
        tp, fp, fn = np.cumsum(call[t][o] & pos[t][o]), np.cumsum(call[t][o] & ~pos[t][o]), np.cumsum(pos[t][o] & ~call[t][o])
        risk = e / k
        aurc[t] = risk.mean()
        for c in kcuts:
            tn = c - tp[c - 1] - fp[c - 1] - fn[c - 1]
            with np.errstate(divide="ignore", invalid="ignore"):
                (risk[c - 1], tp[c - 1] / (tp[c - 1] + fn[c - 1]), tn / (tn + fp[c - 1]), tp[c - 1] / (tp[c - 1] + fp[c - 1]),
                 tn / (tn + fn[c - 1]))
        ends = np.nonzero(np.append(ks[1:] != ks[:-1], True))[0]      # a threshold cuts between tie groups
        for rho in risks:
            ok = ends[risk[ends] <= rho]
            (ok[-1] + 1) / n if ok.size else 0.0
    return aurc


def time_loop(preds, targets, replicates, seed):
    N = targets.shape[0]
    key = selective.keys(preds, "msp").cpu().numpy()
    yhat = selective.predicted(preds).cpu().numpy()
    y = targets.cpu().numpy()
    sel = np.array(selective.CLS_WEIGHTS)[None, :]
    err, pos, call = (yhat != y).T.copy(), (y == sel).T.copy(), (yhat == sel).T.copy()
    kcuts = selective.coverage_cuts(N, selective.check_coverages(selective.DEFAULT_COVERAGES)[1])
    risks = [float(r) for r in selective.DEFAULT_RISKS]
    aurc0 = loop_replicate(key, err, pos, call, multiplicities(seed, 0, N), kcuts, risks)  # warm-up, and the check
    t0 = time.perf_counter()
    for r in range(replicates):
        loop_replicate(key, err, pos, call, multiplicities(seed, r, N), kcuts, risks)
    return (time.perf_counter() - t0) / replicates, aurc0


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("selective_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    records = []
    for N in args.sizes:
        preds, targets = make_inputs(N, args.seed + N, dev)
        rec = {"N": N, "bootstrap": args.bootstrap}
        if args.only in ("both", "report"):
            rec.update(time_report(preds, targets, args.bootstrap, args.seed, args.repeats))
        if args.only in ("both", "loop"):
            per, aurc0 = time_loop(preds, targets, args.loop_replicates, args.seed)
            one = selective.selective_report(preds, targets, bootstrap=1, seed=args.seed)
            rec.update({"loop_s_per_replicate": per, "loop_s_scaled": per * args.bootstrap,
                        "loop_replicates_timed": args.loop_replicates,
                        "max_abs_aurc_difference_replicate_0": float(np.abs(one["summary_replicates"][0, 0, :8].numpy() - aurc0).max())})
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
