"""Times the two kernels of sm3hip.tta and splits one tta.predict pass into its parts.

    python tools/tta_bench.py --out profiles/tta_measure.json

  * dihedral: tta.dihedral(x, "d4") at x [64, 3, 224, 224] against the same tensor made by torch -- torch.stack of the eight
    flip / transpose(...).contiguous() expressions -- alternating the two inside one loop, device events around each call, the
    median and the quartiles of --repeats calls after a warm-up of both; the two results are compared bit for bit first.
  * reduce: tta.reduce at B = 395 (derm7pt's test split), V = 8 and V = 40: the whole call (the finite check, the launch, the
    int64 casts of the three class tensors) between device synchronisations, and the sm3_tta_reduce launch alone with device events.
  * predict: one tta.predict pass of 64 pairs at 224^2 under d4 on the ResNet-50 Baseline (--amp-dtype arithmetic, random weights),
    whole, and its three parts timed apart at the same shapes: the two dihedral calls, the two encoder forwards plus the heads on
    the 512 view pairs, and the reduction."""
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

from sm3hip import ops, tta  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser(description="the kernels of sm3hip.tta and the parts of one predict pass (MI355X)")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--size", type=int, default=224)
    p.add_argument("--cases", type=int, default=395)
    p.add_argument("--repeats", type=int, default=50)
    p.add_argument("--predict-repeats", type=int, default=5)
    p.add_argument("--arch", type=str, default="resnet50")
    p.add_argument("--amp-dtype", choices=("f32", "bf16", "fp16"), default="bf16")
    p.add_argument("--only", choices=("all", "kernels"), default="all")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", type=str, default=None, help="JSON file of the result records")
    return p


def torch_dihedral(x):
    """What a user writes without the kernel: the eight views one after another, stacked."""
    views = []
    for g in range(8):
        v = x.transpose(-1, -2) if g & 4 else x
        if g & 2:
            v = v.flip(-2)
        if g & 1:
            v = v.flip(-1)
        views.append(v.contiguous())
    return torch.stack(views, dim=1)


def _event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def _summary(times):
    q = statistics.quantiles(times, n=4)
    return {"median_s": statistics.median(times), "q1_s": q[0], "q3_s": q[2], "min_s": min(times), "max_s": max(times)}


def _host_time(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return _summary(times)


def bench_dihedral(args, dev):
    g = torch.Generator(device=dev).manual_seed(args.seed)
    x = torch.randn(args.batch, 3, args.size, args.size, device=dev, generator=g)
    ours, theirs = lambda: tta.dihedral(x, "d4"), lambda: torch_dihedral(x)
    if not torch.equal(ours().view(torch.int32), theirs().view(torch.int32)):
        raise SystemExit("tta_bench: tta.dihedral and the torch composition differ")
    for _ in range(3):
        ours(), theirs()
    torch.cuda.synchronize()
    t_ours, t_theirs = [], []
    for _ in range(args.repeats):  # alternating: both see the same neighbours on the machine
        t_ours.append(_event_time(ours))
        t_theirs.append(_event_time(theirs))
    nbytes = 4.0 * x.numel() * 9  # one read, eight stores
    rec = {"what": "dihedral", "shape": list(x.shape), "group": "d4", "repeats": args.repeats, "bytes_moved": nbytes,
           "hip": _summary(t_ours), "torch": _summary(t_theirs)}
    rec["hip_bytes_per_s"] = nbytes / rec["hip"]["median_s"]
    rec["torch_over_hip"] = rec["torch"]["median_s"] / rec["hip"]["median_s"]
    return rec


def bench_reduce(args, dev, V):
    g = torch.Generator(device=dev).manual_seed(args.seed + V)
    z = 4.0 * torch.randn(args.cases, V, 24, device=dev, generator=g)
    B, T = args.cases, 8
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    bufs = [new((B, V, 24), torch.int64), new((B, 24), torch.int64), new((B, 24), torch.int64), new((B, 24), torch.int64),
            new((B, V, T), torch.int32), new((B, T), torch.int32), new((B, T), torch.int32), new((B, 24), torch.float32)]
    launch = lambda: ops.tta_reduce(z, *bufs)
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    return {"what": "reduce", "B": B, "V": V, "repeats": args.repeats, "call": _host_time(lambda: tta.reduce(z), args.repeats),
            "launch": _summary([_event_time(launch) for _ in range(args.repeats)])}


def bench_predict(args, dev):
    from src.models.baseline import Baseline
    torch.manual_seed(args.seed)
    model = Baseline(args.arch, None)
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[args.amp_dtype]
    for b in (model.derm_backbone, model.clinic_backbone):
        b.sm3_dtype = dt
    model.to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(args.seed)
    derm = torch.randn(args.batch, 3, args.size, args.size, device=dev, generator=g)
    clinic = torch.randn(args.batch, 3, args.size, args.size, device=dev, generator=g)
    rec = {"what": "predict", "pairs": args.batch, "size": args.size, "group": "d4", "arch": args.arch, "dtype": args.amp_dtype,
           "repeats": args.predict_repeats}
    out = {}

    def whole():
        out["rec"] = tta.predict(model, derm, clinic, "d4")
    rec["whole"] = _host_time(whole, args.predict_repeats)
    from sm3hip.explain import Subject
    sub = Subject(model, "tta_bench").check(derm, clinic, "pred")
    views = {}

    def make_views():
        views["d"], views["c"] = tta.dihedral(derm, "d4"), tta.dihedral(clinic, "d4")
    rec["views"] = _host_time(make_views, args.predict_repeats)

    def encoders():
        with torch.no_grad(), ops.stream_scope():
            views["logits"] = tta._view_logits(sub, views["d"], views["c"], tta._forward_rows(None, 8))
    rec["encoders_and_heads"] = _host_time(encoders, args.predict_repeats)
    rec["reduce"] = _host_time(lambda: tta.reduce(views["logits"]), args.predict_repeats)
    rec["pairs_per_s"] = args.batch / rec["whole"]["median_s"]
    return rec


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tta_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    records = [bench_dihedral(args, dev), bench_reduce(args, dev, 8), bench_reduce(args, dev, 40)]
    if args.only == "all":
        records.append(bench_predict(args, dev))
    for rec in records:
        print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
    return records


if __name__ == "__main__":
    main()
