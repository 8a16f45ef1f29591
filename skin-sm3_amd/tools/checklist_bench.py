"""Times sm3hip.checklist.checklist_report(bootstrap=B) against the loop a user could write with numpy and scikit-learn: per
replicate roc_auc_score of the five rankings with the replicate's multiplicities as sample_weight, one confusion_matrix per
shown cut of both scores and cohen_kappa_score(weights="quadratic") -- at N = 395 (derm7pt's test split) and at N = MAX_CASES.

    python tools/checklist_bench.py --bootstrap 2000 --loop-replicates 20 --out profiles/checklist_measure.json

The report is timed whole (per-case plumbing, ranking, launches, the copy back and the host's values and order statistics),
between device synchronisations, the median of --repeats calls after a warm-up call; the launches alone are timed with device
events.  Beside them, with the same events, N and B:
  * the launches of sm3_report_counts (evaluation_report's kernel, which this change leaves as it was): the yardstick for "a
    fifth kernel of the same family";
  * the two grids of sm3_checklist_counts: the B replicates in launches of 256 (one workgroup per replicate and part) and in
    launches of DEFAULT_CHUNK (one workgroup per replicate), and the point estimate.
The loop is timed over --loop-replicates replicates after a warm-up and scaled to B (every replicate costs the same); it is fed
the multiplicities of the report's own replicates (Philox4x32-10 restated in numpy, tools/operating_bench.py), and the five AUCs
of its first replicate are held against the report's as a check that both sides compute the same thing.

    python tools/checklist_bench.py --grid-sweep build/checklist_grids --out profiles/checklist_grid_sweep.json

--grid-sweep DIR times the two grids against each other at one launch size: csrc/checklist.hip is built twice into DIR as a
library of its own (unless the two are already there), with -DSM3_CHECKLIST_SPLIT_SLOTS=0 (always one workgroup per replicate,
"one_us") and =2^40 (always one per replicate and part, "four_us"), and called through ctypes, alternating the two: per (N, c)
device events around `launches_per_window` back-to-back launches, median, min and max of 5 windows after a warm-up window,
microseconds per launch; the outputs of the two are held equal."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
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
from sm3hip import checklist, ops, report  # noqa: E402

SPLIT_CHUNK = 256  # the longest launch that sm3_checklist_counts runs as one workgroup per (replicate, part)


def get_parser():
    p = argparse.ArgumentParser(description="checklist_report(bootstrap=B) against a numpy / scikit-learn resampling loop (MI355X)")
    p.add_argument("--bootstrap", type=int, default=2000)
    p.add_argument("--sizes", type=int, nargs="*", default=[395, report.MAX_CASES])
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--loop-replicates", type=int, default=20)
    p.add_argument("--only", choices=("both", "report", "loop"), default="both")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", type=str, default=None, help="JSON file of the result records")
    p.add_argument("--grid-sweep", metavar="DIR", default=None,
                   help="time the two grids of sm3_checklist_counts against each other; DIR holds the two variant libraries")
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
    checklist.checklist_report(preds, targets, bootstrap=B, seed=seed)  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        checklist.checklist_report(preds, targets, bootstrap=B, seed=seed)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    dev = targets.device
    packed, order, gs, ge = checklist.case_inputs(preds, targets, list(checklist.DEFAULT_THRESHOLDS))[:4]
    out = torch.empty((B, checklist.RECORD), dtype=torch.int64, device=dev)

    def launches(chunk):
        def run():
            for r0 in range(0, B, chunk):
                ops.checklist_counts(packed, order, gs, ge, out[r0:r0 + min(chunk, B - r0)], seed, r0)
        return run
    whole = _events(launches(checklist.DEFAULT_CHUNK), repeats)
    split = _events(launches(SPLIT_CHUNK), repeats)
    point = _events(lambda: ops.checklist_counts(packed, order, gs, ge, out[:1], seed, 0, point=True), repeats)
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
            "checklist_launches_s": whole, "launch_share": whole / statistics.median(times),
            "checklist_launches_of_256_s": split, "checklist_point_launch_s": point, "report_counts_launches_s": yard,
            "checklist_over_report_counts": whole / yard, "repeats": repeats}


def loop_replicate(rank, mel, m, thresholds):
    """What a user writes on numpy and scikit-learn for one replicate; returns the five AUCs (0 where one class is not drawn)."""
    from sklearn.metrics import cohen_kappa_score, confusion_matrix, roc_auc_score
    keep = m > 0
    w, yb = m[keep], mel[keep]
    auc = np.zeros(len(rank))
    if yb.any() and not yb.all():
        for i, s in enumerate(rank.values()):
            auc[i] = roc_auc_score(yb, s[keep], sample_weight=w)
    for name in ("hard", "annotated"):
        for k in thresholds:
            confusion_matrix(yb, rank[name][keep] >= k, labels=[False, True], sample_weight=w)
    sh, st = rank["hard"][keep], rank["annotated"][keep]
    cohen_kappa_score(sh, st, labels=list(range(checklist.NS)), weights="quadratic", sample_weight=w)
    float((w * np.abs(sh - st)).sum()) / float(w.sum())
    return auc


def time_loop(preds, targets, replicates, seed):
    N = targets.shape[0]
    th = list(checklist.DEFAULT_THRESHOLDS)
    pi = checklist.score_distribution(preds)
    rank = {"hard": checklist.predicted_scores(preds), "annotated": checklist.true_scores(targets),
            "expected": checklist.expected_score(preds), "tail": checklist.tail_probability(pi, th[0]),
            "diag": torch.softmax(preds[0].double(), 1)[:, 2]}
    rank = {k: v.cpu().numpy() for k, v in rank.items()}
    mel = (targets[:, checklist.MELANOMA[0]] == checklist.MELANOMA[1]).cpu().numpy()
    auc0 = loop_replicate(rank, mel, multiplicities(seed, 0, N), th)  # warm-up, and the check against the report
    t0 = time.perf_counter()
    for r in range(replicates):
        loop_replicate(rank, mel, multiplicities(seed, r, N), th)
    return (time.perf_counter() - t0) / replicates, auc0


GRID_VARIANTS = {"one": 0, "four": 1 << 40}  # SM3_CHECKLIST_SPLIT_SLOTS of each
SWEEP_SIZES = (395, 2000, report.MAX_CASES)
SWEEP_LAUNCHES = ((1, 1), (1, 0), (16, 0), (64, 0), (128, 0), (256, 0), (512, 0), (1024, 0), (2000, 0), (4096, 0))  # (c, point)


def build_grid_variants(folder):
    """DIR/libck_one.so and DIR/libck_four.so from csrc/checklist.hip; a library that is there is kept."""
    csrc = os.path.join(ROOT_PATH, "csrc")
    os.makedirs(folder, exist_ok=True)
    paths = {}
    for name, slots in GRID_VARIANTS.items():
        paths[name] = os.path.join(folder, f"libck_{name}.so")
        if not os.path.exists(paths[name]):
            subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                                   "-munsafe-fp-atomics", "-Wall", "-Wno-unused-function", f"-DSM3_CHECKLIST_SPLIT_SLOTS={slots}",
                                   "-shared", os.path.join(csrc, "checklist.hip"), "-o", paths[name]])
    return paths


def grid_sweep(folder, seed):
    libs = {}
    for name, path in build_grid_variants(folder).items():
        lib = C.CDLL(path)
        lib.sm3_checklist_counts.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_void_p]
        lib.sm3_checklist_counts.restype = C.c_int
        libs[name] = lib
    dev = torch.device("cuda", 0)
    records = []
    for N in SWEEP_SIZES:
        preds, targets = make_inputs(N, seed + N, dev)
        packed, order, gs, ge = checklist.case_inputs(preds, targets, list(checklist.DEFAULT_THRESHOLDS))[:4]
        outs = {v: torch.zeros(max(c for c, _ in SWEEP_LAUNCHES), checklist.RECORD, dtype=torch.int64, device=dev) for v in libs}
        stream = torch.cuda.current_stream().cuda_stream
        for c, point in SWEEP_LAUNCHES:
            reps = max(20, min(2000, 200000 // (c * max(1, N // 400))))
            t = {v: [] for v in libs}
            for window in range(6):
                for v, lib in libs.items():  # alternating the two versions
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(reps):
                        rc = lib.sm3_checklist_counts(packed.data_ptr(), order.data_ptr(), gs.data_ptr(), ge.data_ptr(),
                                                      outs[v].data_ptr(), N, seed + 7, 0, c, point, stream)
                        if rc:
                            raise SystemExit(f"checklist_bench: sm3_checklist_counts returned {rc}")
                    b.record()
                    torch.cuda.synchronize()
                    if window:  # the first window is the warm-up
                        t[v].append(a.elapsed_time(b) * 1e3 / reps)
            if not torch.equal(outs["one"][:c], outs["four"][:c]):
                raise SystemExit(f"checklist_bench: the two grids differ at N = {N}, c = {c}")
            rec = {"N": N, "c": c, "point": point, "launches_per_window": reps}
            for v in libs:
                rec.update({f"{v}_us": statistics.median(t[v]), f"{v}_minmax": [min(t[v]), max(t[v])]})
            print(json.dumps(rec), flush=True)
            records.append(rec)
    return records


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("checklist_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    records = grid_sweep(args.grid_sweep, args.seed) if args.grid_sweep else []
    if args.grid_sweep:
        args.sizes = []
    for N in args.sizes:
        preds, targets = make_inputs(N, args.seed + N, dev)
        rec = {"N": N, "bootstrap": args.bootstrap}
        if args.only in ("both", "report"):
            rec.update(time_report(preds, targets, args.bootstrap, args.seed, args.repeats))
        if args.only in ("both", "loop"):
            per, auc0 = time_loop(preds, targets, args.loop_replicates, args.seed)
            one = checklist.checklist_report(preds, targets, bootstrap=1, seed=args.seed)
            rec.update({"loop_s_per_replicate": per, "loop_s_scaled": per * args.bootstrap,
                        "loop_replicates_timed": args.loop_replicates,
                        "max_abs_auc_difference_replicate_0": float(np.abs(one["replicates"][0, :5, 0].numpy() - auc0).max())})
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
