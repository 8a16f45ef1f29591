"""Times sm3hip.operating.operating_report(bootstrap=B) against the loop a user could write with scikit-learn: per replicate and
column one roc_curve and one precision_recall_curve with the replicate's multiplicities as sample_weight (2 x 24 host calls per
replicate), and from them AP, the Youden and F1 optima, sensitivity at the specificity floors and specificity at the
sensitivity floors -- at N = 395 (derm7pt's test split) and at N = MAX_CASES.

    python tools/operating_bench.py --bootstrap 2000 --loop-replicates 20 --out profiles/operating_measure.json

The report is timed whole (ranking, launches, the copy back and the host's values, averages and order statistics), between
device synchronisations, the median of --repeats calls after a warm-up call; the launches alone are timed with device events,
and their share of the whole is recorded.  The loop is timed over --loop-replicates replicates after a warm-up and scaled to B
(every replicate costs the same); it is fed the multiplicities of the report's own replicates (Philox4x32-10 restated in numpy
below), and the AP of its first replicate is held against the report's as a check that both sides compute the same thing.
Both sides see the same seeded predictions with tied scores."""
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

from sm3hip import metrics, operating, ops, report  # noqa: E402

M32 = np.uint64(0xFFFFFFFF)


def get_parser():
    p = argparse.ArgumentParser(description="operating_report(bootstrap=B) against a scikit-learn resampling loop (MI355X)")
    p.add_argument("--bootstrap", type=int, default=2000)
    p.add_argument("--sizes", type=int, nargs="*", default=[395, report.MAX_CASES])
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--loop-replicates", type=int, default=20)
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


def multiplicities(seed, r, N):
    """m_r [N] of the reports' replicate r: draw d hits case (w * N) >> 32, w = word d % 4 of Philox4x32-10 with key = the seed and
    counter (d // 4, r, 0, 2)."""
    c0 = np.arange((N + 3) // 4, dtype=np.uint64)
    c1, c2, c3 = (np.full_like(c0, v) for v in (r, 0, 2))
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & M32, p0 & M32, n0, n2
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    w = np.stack([c0, c1, c2, c3], axis=1).reshape(-1)[:N]
    return np.bincount(((w * np.uint64(N)) >> np.uint64(32)).astype(np.int64), minlength=N).astype(np.int64)


def time_report(preds, targets, B, seed, repeats):
    operating.operating_report(preds, targets, bootstrap=B, seed=seed)  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        operating.operating_report(preds, targets, bootstrap=B, seed=seed)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    # the launches alone, by device events
    dev = targets.device
    order, gs, ge, _ = report.ranking(preds, targets)
    y = targets.int().contiguous()
    colmap = torch.tensor(report.COLUMN_PAIRS, dtype=torch.int32, device=dev)
    sigma = torch.tensor([operating.q32_floor(s) for s in operating.DEFAULT_SPEC], dtype=torch.int64, device=dev)
    rho = torch.tensor([operating.q32_floor(s) for s in operating.DEFAULT_SENS], dtype=torch.int64, device=dev)
    Lt = len(operating.DEFAULT_DECISION)
    fixpos = torch.full((report.K, Lt), targets.shape[0] // 2, dtype=torch.int32, device=dev)
    out = torch.empty((B, report.K, ops.operating_record(3, 3, Lt)), dtype=torch.int64, device=dev)
    kern = []
    for _ in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for r0 in range(0, B, operating.DEFAULT_CHUNK):
            ops.operating_counts(order, gs, ge, y, colmap, sigma, rho, fixpos, out[r0:r0 + min(operating.DEFAULT_CHUNK, B - r0)],
                                 seed, r0)
        b.record()
        torch.cuda.synchronize()
        kern.append(a.elapsed_time(b) / 1e3)
    return statistics.median(times), min(times), max(times), statistics.median(kern[1:])


def loop_replicate(scores, ybin, m):
    """What a user writes on scikit-learn: per column the two curves under the multiplicities, then the searches.  Returns the
    24 average precisions (0 where a class has no positive or no negative among the drawn cases)."""
    from sklearn.metrics import precision_recall_curve, roc_curve
    keep = m > 0
    w = m[keep]
    ap = np.zeros(len(scores))
    for k, (s, yb) in enumerate(zip(scores, ybin)):
        s, yb = s[keep], yb[keep]
        pos = int(w[yb].sum())
        if pos == 0 or pos == int(w.sum()):
            continue
        fpr, tpr, _ = roc_curve(yb, s, sample_weight=w, drop_intermediate=False)
        prec, rec, _ = precision_recall_curve(yb, s, sample_weight=w)
        ap[k] = -np.sum(np.diff(rec) * prec[:-1])
        np.max(tpr - fpr)
        with np.errstate(divide="ignore", invalid="ignore"):
            np.nanmax(2 * prec * rec / (prec + rec))
        for s0 in operating.DEFAULT_SPEC:
            tpr[1 - fpr >= s0].max()
        for r0 in operating.DEFAULT_SENS:
            (1 - fpr)[tpr >= r0].max()
    return ap


def time_loop(preds, targets, replicates, seed):
    N = targets.shape[0]
    scores = [torch.softmax(preds[t].double(), 1)[:, c].cpu().numpy() for t, c in report.COLUMN_PAIRS]
    ybin = [(targets[:, t] == c).cpu().numpy() for t, c in report.COLUMN_PAIRS]
    ap0 = loop_replicate(scores, ybin, multiplicities(seed, 0, N))  # warm-up, and the check against the report
    t0 = time.perf_counter()
    for r in range(replicates):
        loop_replicate(scores, ybin, multiplicities(seed, r, N))
    return (time.perf_counter() - t0) / replicates, ap0


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("operating_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    records = []
    for N in args.sizes:
        preds, targets = make_inputs(N, args.seed + N, dev)
        rec = {"N": N, "bootstrap": args.bootstrap}
        if args.only in ("both", "report"):
            med, lo, hi, kern = time_report(preds, targets, args.bootstrap, args.seed, args.repeats)
            rec.update({"report_s": med, "report_s_min": lo, "report_s_max": hi, "report_launches_s": kern,
                        "launch_share": kern / med, "repeats": args.repeats})
        if args.only in ("both", "loop"):
            per, ap0 = time_loop(preds, targets, args.loop_replicates, args.seed)
            one = operating.operating_report(preds, targets, bootstrap=1, seed=args.seed)
            rec.update({"loop_s_per_replicate": per, "loop_s_scaled": per * args.bootstrap,
                        "loop_replicates_timed": args.loop_replicates,
                        "max_abs_ap_difference_replicate_0": float(np.abs(one["replicates"][0, 0, :report.K].numpy() - ap0).max())})
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
