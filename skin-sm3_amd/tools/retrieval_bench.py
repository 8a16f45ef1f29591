"""Times sm3hip.retrieval.cross_modal_report(bootstrap=B) against the loop a user could write without it: per replicate, resample
the cases on the GPU, gather the resampled similarity matrix and rank every positive in torch -- at N = 395 (derm7pt's test
split) and at N = MAX_CASES, on random unit-norm embeddings of width 128 whose pairs share a signal.

    python tools/retrieval_bench.py --bootstrap 2000 --loop-replicates 40 --out profiles/retrieval_measure.json

The report is timed whole (normalisation, both similarity matrices, all launches, the copy back and the host's values and order
statistics), between device synchronisations, after a warm-up call; its kernel launches alone (2 x beats, 2 x counts, on buffers
allocated beforehand, nothing copied back) are timed with device events, and the counts kernel's popcount rate is the popcounts
its replicates execute over that time.  The loop is timed over --loop-replicates replicates after a warm-up and scaled to B
(every replicate costs the same); it is handed the similarity matrix ready-made.  Report and loop alternate, --repeats times;
the medians are reported.
Kernel time comes from a separate run under rocprofv3 --kernel-trace --stats with --only report."""
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

from sm3hip import retrieval  # noqa: E402
from sm3hip.knn import normalize  # noqa: E402

KS = (1, 5, 10)


def get_parser():
    p = argparse.ArgumentParser(description="cross_modal_report(bootstrap=B) against a torch resampling loop (MI355X)")
    p.add_argument("--bootstrap", type=int, default=2000)
    p.add_argument("--sizes", type=int, nargs="*", default=[395, retrieval.MAX_CASES])
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--loop-replicates", type=int, default=40)
    p.add_argument("--only", choices=("both", "report", "loop"), default="both")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", type=str, default=None, help="JSON file of the result records")
    return p


def make_inputs(N, D, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    base = torch.randn(N, D, device=dev, generator=g)
    return (normalize(base + 1.5 * torch.randn(N, D, device=dev, generator=g)),
            normalize(base + 1.5 * torch.randn(N, D, device=dev, generator=g)))


def time_report(zd, zc, B, seed):
    t0 = time.perf_counter()
    retrieval.cross_modal_report(zd, zc, ks=KS, bootstrap=B, seed=seed)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def time_launches(zd, zc, B, seed):
    """(beats seconds, counts seconds) of the two directions' kernel launches alone, by device events: both similarity matrices,
    the packed flags and the records are allocated and S is multiplied before the first event; nothing is copied back between
    the events."""
    from sm3hip import ops
    from sm3hip.knn import KNNBank
    N, D = zd.shape
    dev = zd.device
    W = (N + 31) // 32
    sides = []
    for q, g in ((zd, zc), (zc, zd)):
        bank = KNNBank(g, torch.zeros(N, dtype=torch.int32, device=dev), 1)
        S = torch.empty(N, bank.ld, dtype=torch.float32, device=dev)
        bank.similarity(q.contiguous() if bank.Dp == D else torch.nn.functional.pad(q, (0, bank.Dp - D)), S)
        sides.append((S, torch.empty(N, W, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev),
                      torch.empty(N, dtype=torch.float64, device=dev), torch.empty(B, len(KS) + 3, dtype=torch.int64, device=dev)))
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    for S, bits, rank, term, _ in sides:
        ops.retrieval_beats(S, 0, N, 0.1, bits, rank, term)
    ev[1].record()
    for _, bits, _, _, out in sides:
        for r0 in range(0, B, retrieval.DEFAULT_CHUNK):
            ops.retrieval_counts(bits, KS, out[r0:r0 + min(retrieval.DEFAULT_CHUNK, B - r0)], seed, r0)
    ev[2].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / 1e3, ev[1].elapsed_time(ev[2]) / 1e3


def popcounts(seed, B, N):
    """The popcounts sm3_retrieval_counts executes for replicates 0 .. B - 1 of one direction: per replicate (cases drawn at least
    once) x W words x P planes, P = the bits of the largest multiplicity -- from the multiplicities themselves (Philox4x32-10, key
    = the seed, counter (d / 4, r, 0, 2), case (w N) >> 32), restated here in numpy."""
    import numpy as np
    M32 = np.uint64(0xFFFFFFFF)
    W, total = (N + 31) // 32, 0
    for r0 in range(0, B, 64):
        r = np.arange(r0, min(r0 + 64, B), dtype=np.uint64)[:, None]
        c0 = np.broadcast_to(np.arange((N + 3) // 4, dtype=np.uint64)[None, :], (r.shape[0], (N + 3) // 4)).copy()
        c1, c2, c3 = np.broadcast_to(r, c0.shape).copy(), np.zeros_like(c0), np.full_like(c0, 2)
        k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
        for _ in range(10):
            p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
            n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
            c1, c3, c0, c2 = p1 & M32, p0 & M32, n0, n2
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
        w = np.stack([c0, c1, c2, c3], axis=2).reshape(r.shape[0], -1)[:, :N]
        idx = ((w * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
        for row in idx:
            m = np.bincount(row, minlength=N)
            total += int((m > 0).sum()) * W * int(m.max()).bit_length()
    return total


def loop_replicate(S, gen):
    """What a user writes in torch: resample the cases, rank every positive (copies of a case are its positive, the lower case
    index wins a tie), R@k, mean and median rank, MRR."""
    N = S.shape[0]
    idx = torch.randint(0, N, (N,), device=S.device, generator=gen)
    Sr = S[idx][:, idx]
    d = S[idx, idx][:, None]
    other = idx[None, :] != idx[:, None]
    rho = (other & ((Sr > d) | ((Sr == d) & (idx[None, :] < idx[:, None])))).sum(dim=1)
    out = [(rho < k).double().mean() for k in KS]
    return out + [rho.double().mean() + 1, rho.median() + 1, (1.0 / (rho + 1).double()).mean()]


def time_loop(zd, zc, replicates, seed):
    S = zd @ zc.t()
    gen = torch.Generator(device=S.device).manual_seed(seed)
    for _ in range(2):
        loop_replicate(S, gen), loop_replicate(S.t(), gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replicates):
        loop_replicate(S, gen), loop_replicate(S.t(), gen)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / replicates


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    records = []
    for N in args.sizes:
        zd, zc = make_inputs(N, args.dim, args.seed + N, dev)
        rec = {"N": N, "D": args.dim, "bootstrap": args.bootstrap, "repeats": args.repeats}
        rep_t, loop_t, beats_t, counts_t = [], [], [], []
        if args.only in ("both", "report"):
            time_report(zd, zc, args.bootstrap, args.seed)  # warm-up: code objects, allocator
            time_launches(zd, zc, args.bootstrap, args.seed)
        for _ in range(args.repeats):  # alternating
            if args.only in ("both", "report"):
                rep_t.append(time_report(zd, zc, args.bootstrap, args.seed))
                b, c = time_launches(zd, zc, args.bootstrap, args.seed)
                beats_t.append(b)
                counts_t.append(c)
            if args.only in ("both", "loop"):
                loop_t.append(time_loop(zd, zc, args.loop_replicates, args.seed))
        if rep_t:
            pops = 2.0 * popcounts(args.seed, args.bootstrap, N)  # both directions share the multiplicities
            rec.update({"report_s": statistics.median(rep_t), "report_s_min": min(rep_t), "report_s_max": max(rep_t),
                        "beats_launches_s": statistics.median(beats_t), "counts_launches_s": statistics.median(counts_t),
                        "report_launches_s": statistics.median(beats_t) + statistics.median(counts_t),
                        "counts_popcounts": pops, "counts_popcounts_per_s": pops / statistics.median(counts_t)})
        if loop_t:
            per = statistics.median(loop_t)
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
