"""Times sm3hip.tsne.tsne() against scikit-learn's TSNE(method="exact") on the same points: paired unit-norm embeddings of width
128 (N / 2 cases in five islands, two modalities each), at N = 790 (the two modalities of derm7pt's 395 test cases) and N = 2022
(all 1011 cases); at N = MAX_POINTS tsne() alone (the exact CPU method would take hours there).

    python tools/tsne_bench.py --out profiles/tsne_measure.json
    rocprofv3 --kernel-trace --stats --output-format csv -d out -o tsne -- python tools/tsne_bench.py --only tsne --sizes 2022 --big 0

tsne() is timed end to end -- the copy of the first map to the device, the affinities, every launch, the checks' copies back and
the final map's -- by the host clock around a final device synchronise, after a warm-up call on the same shape; --repeats times,
the median is reported beside every value.  scikit-learn runs once per size on the CPU with the same perplexity, iterations and
init="random".  Both report their final KL, so the two maps can be seen to be of one quality.  Kernel time comes from a separate
run under rocprofv3 --kernel-trace --stats with --only tsne (tracing slows the host)."""
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

from sm3hip import tsne  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser(description="tsne() against scikit-learn's exact t-SNE (MI355X)")
    p.add_argument("--sizes", type=int, nargs="*", default=[790, 2022], help="points, timed for both")
    p.add_argument("--big", type=int, default=tsne.MAX_POINTS, help="points, timed for tsne() alone (0: skip)")
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--perplexity", type=float, default=30.0)
    p.add_argument("--iters", type=int, default=1000)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--only", choices=("both", "tsne", "sklearn"), default="both")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", type=str, default=None, help="JSON file of the result records")
    return p


def make_inputs(N, D, seed):
    """[N, D] float32 on the CPU: N // 2 cases (the rest of an odd N: one more), each a point of one of five islands, seen twice
    with independent noise, every row of unit norm; from a CPU generator, so the same values everywhere."""
    g = torch.Generator().manual_seed(seed)
    cases = (N + 1) // 2
    centres = 2.0 * torch.randn(5, D, generator=g)
    base = centres[torch.arange(cases) % 5] + torch.randn(cases, D, generator=g)
    x = torch.cat([base + 0.5 * torch.randn(cases, D, generator=g), base + 0.5 * torch.randn(cases, D, generator=g)])[:N]
    return torch.nn.functional.normalize(x, dim=1).contiguous()


def time_tsne(x, settings):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rep = tsne.tsne(x, **settings)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, rep


def time_sklearn(x, args):
    from sklearn.manifold import TSNE
    t = TSNE(method="exact", init="random", perplexity=args.perplexity, max_iter=args.iters, random_state=args.seed)
    t0 = time.perf_counter()
    t.fit(x.numpy())
    return time.perf_counter() - t0, float(t.kl_divergence_), int(t.n_iter_)


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not torch.cuda.is_available() and args.only != "sklearn":
        raise SystemExit("tsne_bench: needs a GPU")
    settings = dict(perplexity=args.perplexity, iters=args.iters, seed=args.seed)
    records = []
    for N in list(args.sizes) + ([args.big] if args.big else []):
        both = N in args.sizes
        x = make_inputs(N, args.dim, args.seed)
        rec = {"N": N, "D": args.dim, "perplexity": args.perplexity, "iters": args.iters}
        if args.only != "sklearn":
            xd = x.cuda()
            time_tsne(xd, {**settings, "iters": min(args.iters, 20)})  # warm-up on this shape: code objects, the allocator
            times, rep = [], None
            for _ in range(args.repeats if both else 1):
                t, rep = time_tsne(xd, settings)
                times.append(t)
            rec.update(tsne_s=statistics.median(times), tsne_s_all=times, tsne_kl=rep["kl"], tsne_iters_run=rep["iters_run"],
                       device=torch.cuda.get_device_name(0))
        if both and args.only != "tsne":
            import sklearn
            s, kl, n_iter = time_sklearn(x, args)
            rec.update(sklearn_s=s, sklearn_kl=kl, sklearn_iters_run=n_iter, sklearn=sklearn.__version__,
                       cpu_threads=torch.get_num_threads())
            if "tsne_s" in rec:
                rec["ratio"] = s / rec["tsne_s"]
        records.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/tsne_bench.py", "records": records}, f, indent=1)
            f.write("\n")
    return records


if __name__ == "__main__":
    main()
