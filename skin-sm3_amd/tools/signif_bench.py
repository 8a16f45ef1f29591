"""Times sm3hip.significance.significance_report(permutations=B) against the loop a user could write without it: per replicate,
swap the two models' predictions of a random half of the cases on the host, call sklearn.metrics.roc_auc_score for the 24
one-vs-rest AUCs of both sides and count TP / FP of both sides with numpy -- at N = 395 (derm7pt's test split) and at
N = MAX_CASES.

    python tools/signif_bench.py --permutations 10000 --loop-replicates 20 --out profiles/signif_measure.json

The report is timed whole (the joint ranking, the launches, the copy back, the host's values and p-values, DeLong and McNemar),
between device synchronisations, the median of --repeats calls after a warm-up call; the launches of sm3_signif_counts alone are
timed with device events, and beside them the launches of sm3_report_counts (the bootstrap's kernel) at the same N and B: the
yardstick for "a replicate of 2N joint positions against a replicate of N".  The loop is timed over --loop-replicates replicates
after a warm-up and scaled to B (every replicate costs the same).  Both sides see the same seeded predictions with tied
scores."""
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

from sm3hip import metrics, ops, report, significance  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser(description="significance_report(permutations=B) against a scikit-learn swap loop (MI355X)")
    p.add_argument("--permutations", type=int, default=10000)
    p.add_argument("--sizes", type=int, nargs="*", default=[395, report.MAX_CASES])
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--loop-replicates", type=int, default=20)
    p.add_argument("--only", choices=("both", "report", "loop"), default="both")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", type=str, default=None, help="JSON file of the result records")
    return p


def make_inputs(N, seed, dev):
    """Seeded logits in steps of 1/4 (tied scores, as a saturated classifier gives) of two models, and labels."""
    g = torch.Generator().manual_seed(seed)
    targets = torch.stack([torch.randint(0, n, (N,), generator=g) for n in metrics.NUM_CLASSES], dim=1)
    a = [(4.0 * torch.randn(N, n, generator=g)).round() / 4.0 for n in metrics.NUM_CLASSES]
    b = [(p + torch.randn(p.shape, generator=g)).mul(4.0).round() / 4.0 for p in a]
    return [p.to(dev) for p in a], [p.to(dev) for p in b], targets.to(dev)


def _events(fn, repeats):
    times = []
    for _ in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / 1e3)
    return statistics.median(times[1:])


def time_report(a, b, targets, B, seed, repeats):
    significance.significance_report(a, b, targets, permutations=B, seed=seed)  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        significance.significance_report(a, b, targets, permutations=B, seed=seed)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dev = targets.device
    y = targets.int().contiguous()
    colmap = torch.tensor(report.COLUMN_PAIRS, dtype=torch.int32, device=dev)
    order, gs, ge, ha, hb = significance.joint_ranking(a, b)
    out = torch.empty((B, report.K, 2, 3), dtype=torch.int64, device=dev)

    def signif():
        for r0 in range(0, B, significance.DEFAULT_CHUNK):
            ops.signif_counts(order, gs, ge, y, ha, hb, colmap, out[r0:r0 + min(significance.DEFAULT_CHUNK, B - r0)], seed, r0)
    o1, g1s, g1e, yhat = report.ranking(a, targets)
    rout = torch.empty((B, report.K, 6), dtype=torch.int64, device=dev)

    def yardstick():
        for r0 in range(0, B, report.DEFAULT_CHUNK):
            ops.report_counts(o1, g1s, g1e, y, yhat, colmap, rout[r0:r0 + min(report.DEFAULT_CHUNK, B - r0)], seed, r0)
    place = torch.empty((report.K, targets.shape[0]), dtype=torch.int32, device=dev)
    return (statistics.median(times), min(times), max(times), _events(signif, repeats), _events(yardstick, repeats),
            _events(lambda: ops.signif_placements(o1, g1s, g1e, y, colmap, place), repeats))


def loop_replicate(sa, sb, ha, hb, y, rng):
    """What a user writes on scikit-learn and numpy alone: swap, 48 AUCs, 48 pairs of counts."""
    from sklearn.metrics import roc_auc_score
    swap = rng.random(y.shape[0]) < 0.5
    out = []
    for s, h in ((np.where(swap[None], sb, sa), np.where(swap[:, None], hb, ha)),
                 (np.where(swap[None], sa, sb), np.where(swap[:, None], ha, hb))):
        for k, (t, c) in enumerate(report.COLUMN_PAIRS):
            pos = y[:, t] == c
            out.append((roc_auc_score(pos, s[k]), int((pos & (h[:, t] == c)).sum()), int((~pos & (h[:, t] == c)).sum())))
    return out


def time_loop(a, b, targets, replicates, seed):
    sa, sb = (torch.cat([torch.softmax(p.double(), dim=1).t() for p in preds], dim=0).cpu().numpy() for preds in (a, b))
    ha, hb = (torch.stack([p.argmax(dim=1) for p in preds], dim=1).cpu().numpy() for preds in (a, b))
    y = targets.cpu().numpy()
    rng = np.random.default_rng(seed)
    for _ in range(2):
        loop_replicate(sa, sb, ha, hb, y, rng)
    t0 = time.perf_counter()
    for _ in range(replicates):
        loop_replicate(sa, sb, ha, hb, y, rng)
    return (time.perf_counter() - t0) / replicates


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("signif_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    records = []
    for N in args.sizes:
        a, b, targets = make_inputs(N, args.seed + N, dev)
        rec = {"N": N, "permutations": args.permutations}
        if args.only in ("both", "report"):
            med, lo, hi, kern, yard, place = time_report(a, b, targets, args.permutations, args.seed, args.repeats)
            rec.update({"significance_report_s": med, "significance_report_s_min": lo, "significance_report_s_max": hi,
                        "signif_counts_launches_s": kern, "report_counts_launches_s": yard,
                        "signif_over_report_counts": kern / yard, "signif_placements_launch_s": place, "repeats": args.repeats})
        if args.only in ("both", "loop"):
            per = time_loop(a, b, targets, args.loop_replicates, args.seed)
            rec.update({"loop_s_per_replicate": per, "loop_s_scaled": per * args.permutations,
                        "loop_replicates_timed": args.loop_replicates})
        if "significance_report_s" in rec and "loop_s_scaled" in rec:
            rec["loop_over_significance_report"] = rec["loop_s_scaled"] / rec["significance_report_s"]
        print(json.dumps(rec), flush=True)
        records.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
    return records


if __name__ == "__main__":
    main()
