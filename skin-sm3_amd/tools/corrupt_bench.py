"""Times the four kernels of sm3hip.corrupt against the plain torch composition of the same operation, and one whole
corrupt.predict_split.

    python tools/corrupt_bench.py --out profiles/corrupt_measure.json

  * kernels: corrupt.apply at x [64, 3, 224, 224] for gaussian_noise, impulse_noise, colour_cast (sm3_corrupt_pointwise),
    defocus_blur and motion_blur (sm3_corrupt_taps), pixelate and jpeg, at --severities, against what a user writes in torch --
    clamp(x + sigma * randn_like(x)); two rand_like masks; a broadcast product; conv2d with the disk or line kernel over a
    replicate-padded input; avg_pool2d + repeat_interleave; a float matrix-product DCT on unfolded 8 x 8 blocks (no torch.fft).
    corrupt.apply (the whole call: its host half, the allocation, the launch), the entry point's wrapper alone on tensors and
    tables made beforehand, and the composition alternate inside one loop, device events around each, the median and the
    quartiles of --repeats calls after a warm-up of all three.  The compositions are not bit-equal to the kernels (other random
    streams, float arithmetic, fused sums): the largest difference is reported where the operation is deterministic, nothing
    is asserted.  Reported per kernel: the times, the
    algorithmic bytes (one read and one write of the image) over the launch's for the HBM-bound ones, the integer operations over
    it for jpeg (4 passes x 8 multiply-adds per pixel and channel), and the ratios to the torch composition.
  * predict_split: one corrupt.predict_split of 64 pairs at 224^2 on the ResNet-50 Baseline (--amp-dtype arithmetic, random
    weights) over a random image store, every corruption at --severities, whole; and the corruption kernels of that pass alone
    (every corrupt.apply it makes, on the same tensors), whose share of the whole is reported.
Records of the output file that this tool does not make (the Pillow comparison of tests/test_corrupt_cpu.py) are kept."""
import argparse
import json
import math
import os
import statistics
import sys
import time
from types import SimpleNamespace

SCRIPT_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT_PATH = os.path.split(SCRIPT_DIR)[0]
sys.path.insert(0, ROOT_PATH)

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # kernel arguments in device memory: see sm3hip/__init__.py

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from sm3hip import corrupt, ops  # noqa: E402

KERNEL_OF = {"gaussian_noise": "pointwise", "impulse_noise": "pointwise", "colour_cast": "pointwise", "defocus_blur": "taps",
             "motion_blur": "taps", "pixelate": "pixelate", "jpeg": "jpeg"}


def get_parser():
    p = argparse.ArgumentParser(description="the kernels of sm3hip.corrupt and one predict_split pass (MI355X)")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--size", type=int, default=224)
    p.add_argument("--repeats", type=int, default=30)
    p.add_argument("--predict-repeats", type=int, default=3)
    p.add_argument("--severities", type=int, nargs="+", default=[1, 5])
    p.add_argument("--arch", type=str, default="resnet50")
    p.add_argument("--amp-dtype", choices=("f32", "bf16", "fp16"), default="bf16")
    p.add_argument("--only", choices=("all", "kernels"), default="all")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", type=str, default=None, help="JSON file of the result records")
    return p


# ---- what a user writes in torch ----------------------------------------------------------------------------------------------
def _tap_weight(taps, dev):
    k = torch.zeros(21, 21, device=dev)
    for dy, dx in taps:
        k[10 + int(dy), 10 + int(dx)] += 1.0
    return (k / len(taps))[None, None].repeat(3, 1, 1, 1)


def _dct(dev):
    c = [[(math.sqrt(1 / 8) if k == 0 else math.sqrt(2 / 8)) * math.cos((2 * n + 1) * k * math.pi / 16) for n in range(8)]
         for k in range(8)]
    return torch.tensor(c, device=dev)


def torch_jpeg(x, quality):
    B, _, H, W = x.shape
    dev = x.device
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    q = F.pad((x * 255).round().clamp(0, 255), (0, Wp - W, 0, Hp - H), mode="replicate")
    m = torch.tensor([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]], device=dev)
    ycc = torch.einsum("ij,bjhw->bihw", m, q) + torch.tensor([0.0, 128.0, 128.0], device=dev)[None, :, None, None]
    blocks = (ycc.round() - 128).view(B, 3, Hp // 8, 8, Wp // 8, 8).permute(0, 1, 2, 4, 3, 5)
    C8 = _dct(dev)
    t = torch.stack([torch.from_numpy(a.astype(np.float32)).view(8, 8) for a in corrupt.quant_tables(quality)]).to(dev)
    t = t[[0, 1, 1]][None, :, None, None]
    coef = torch.round(C8 @ blocks @ C8.T / t) * t
    back = (C8.T @ coef @ C8).round().add(128).clamp(0, 255).permute(0, 1, 2, 4, 3, 5).reshape(B, 3, Hp, Wp)[:, :, :H, :W]
    y, cb, cr = back[:, 0], back[:, 1] - 128, back[:, 2] - 128
    rgb = torch.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], dim=1)
    return rgb.round().clamp(0, 255) / 255


def torch_version(x, name, severity, ids, seed):
    """The composition for (name, severity): a function of no arguments, and whether its result is comparable to the kernel's."""
    p, dev = corrupt.parameters(name, severity), x.device
    if name == "gaussian_noise":
        return (lambda: (x + p * torch.randn_like(x)).clamp(0, 1)), False
    if name == "impulse_noise":
        def impulse():
            u = torch.rand_like(x)
            return torch.where(u < p / 2, torch.zeros_like(x), torch.where(u > 1 - p / 2, torch.ones_like(x), x))
        return impulse, False
    if name == "colour_cast":
        cool = torch.from_numpy((corrupt.case_words(ids, name, severity, seed) & 1).astype(bool)).to(dev)
        g = torch.where(cool[:, None], torch.tensor([1 - p, 1.0, 1 + p], device=dev), torch.tensor([1 + p, 1.0, 1 - p], device=dev))
        return (lambda: (x * g[:, :, None, None]).clamp(0, 1)), True
    if name == "defocus_blur":
        w = _tap_weight(corrupt.tap_tables(name, severity)[0][0], dev)
        return (lambda: F.conv2d(F.pad(x, (10, 10, 10, 10), mode="replicate"), w, groups=3)), True
    if name == "motion_blur":
        tables, _ = corrupt.tap_tables(name, severity)
        ks = (corrupt.case_words(ids, name, severity, seed) & 7).astype(np.int64)
        ws = [_tap_weight(tables[k], dev) for k in range(8)]
        groups = [(torch.from_numpy(np.nonzero(ks == k)[0]).to(dev), ws[k]) for k in range(8) if (ks == k).any()]

        def motion():
            out, xp = torch.empty_like(x), F.pad(x, (10, 10, 10, 10), mode="replicate")
            for idx, w in groups:  # one convolution per direction present in the batch
                out[idx] = F.conv2d(xp[idx], w, groups=3)
            return out
        return motion, True
    if name == "pixelate":
        H, W = x.shape[2:]
        return (lambda: F.avg_pool2d(x, p, ceil_mode=True).repeat_interleave(p, 2).repeat_interleave(p, 3)[:, :, :H, :W]), True
    return (lambda: torch_jpeg(x, p)), True


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


def launch_alone(x, ids, name, severity, seed):
    """The entry point's wrapper alone, on tensors and tables made beforehand: what corrupt.apply launches, without its host half."""
    p, out = corrupt.parameters(name, severity), torch.empty_like(x)
    if KERNEL_OF[name] == "pointwise":
        dev_ids = torch.from_numpy(ids.astype(np.int32)).to(x.device)
        param = int(p * 2 ** 31) if name == "impulse_noise" else p
        return lambda: ops.corrupt_pointwise(x, dev_ids, corrupt.CORRUPTIONS[name], severity, param, seed, 0, out)
    if KERNEL_OF[name] == "taps":
        tables, counts = corrupt.tap_tables(name, severity)
        index = (corrupt.case_words(ids, name, severity, seed) & 7).astype(np.int32) if name == "motion_blur" else \
            np.zeros(len(ids), dtype=np.int32)
        return lambda: ops.corrupt_taps(x, tables, counts, index, out)
    if name == "pixelate":
        return lambda: ops.corrupt_pixelate(x, p, out)
    ql, qc = corrupt.quant_tables(p)
    return lambda: ops.corrupt_jpeg(x, p, ql, qc, out)


def bench_kernel(args, dev, x, ids, name, severity):
    ours = lambda: corrupt.apply(x, name, severity, ids, args.seed, 0)
    launch = launch_alone(x, ids, name, severity, args.seed)
    theirs, comparable = torch_version(x, name, severity, ids, args.seed)
    rec = {"what": "kernel", "kernel": "sm3_corrupt_" + KERNEL_OF[name], "name": name, "severity": severity,
           "parameter": corrupt.parameters(name, severity), "shape": list(x.shape), "repeats": args.repeats}
    if comparable:
        rec["max_abs_diff_to_torch"] = float((ours() - theirs()).abs().max())
    for _ in range(3):
        ours(), launch(), theirs()
    torch.cuda.synchronize()
    t_ours, t_launch, t_theirs = [], [], []
    for _ in range(args.repeats):  # alternating: all three see the same neighbours on the machine
        t_ours.append(_event_time(ours))
        t_launch.append(_event_time(launch))
        t_theirs.append(_event_time(theirs))
    rec["hip"], rec["launch"], rec["torch"] = _summary(t_ours), _summary(t_launch), _summary(t_theirs)  # hip: the whole apply call
    rec["torch_over_hip"] = rec["torch"]["median_s"] / rec["hip"]["median_s"]
    rec["torch_over_launch"] = rec["torch"]["median_s"] / rec["launch"]["median_s"]
    if name == "jpeg":
        B, _, H, W = x.shape
        rec["integer_ops"] = float(B * (-(-H // 8) * 8) * (-(-W // 8) * 8) * 3 * 4 * 8 * 2)
        rec["launch_integer_ops_per_s"] = rec["integer_ops"] / rec["launch"]["median_s"]
    rec["bytes_moved"] = 8.0 * x.numel()  # one read and one write of the image
    rec["launch_bytes_per_s"] = rec["bytes_moved"] / rec["launch"]["median_s"]
    return rec


def random_store(n, dev, seed):
    """An image store of n random uint8 images of 300 x 400 and a split pairing image 2i with image 2i + 1."""
    from sm3hip.imagestore import StoreSplit
    g = torch.Generator().manual_seed(seed)
    h, w = 300, 400
    arena = torch.randint(0, 256, (n * h * w * 3,), dtype=torch.uint8, generator=g).to(dev)
    store = SimpleNamespace(arena=arena, offset=torch.arange(n, dtype=torch.int64) * (h * w * 3),
                            img_h=torch.full((n,), h, dtype=torch.int32), img_w=torch.full((n,), w, dtype=torch.int32))
    labels = torch.zeros(n // 2, 8, dtype=torch.int64, device=dev)
    return store, StoreSplit(torch.arange(0, n, 2, dtype=torch.int32), torch.arange(1, n, 2, dtype=torch.int32), labels)


def bench_predict(args, dev):
    from src.models.baseline import Baseline
    torch.manual_seed(args.seed)
    model = Baseline(args.arch, None)
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[args.amp_dtype]
    for b in (model.derm_backbone, model.clinic_backbone):
        b.sm3_dtype = dt
    model.to(dev).eval()
    store, split = random_store(2 * args.batch, dev, args.seed)
    size, mean, std = (args.size, args.size), [0.5] * 3, [0.25] * 3
    names, sev = list(corrupt.CORRUPTIONS), sorted(args.severities)
    rec = {"what": "predict_split", "pairs": args.batch, "size": args.size, "arch": args.arch, "dtype": args.amp_dtype,
           "corruptions": len(names), "severities": sev, "passes": 1 + len(names) * len(sev), "repeats": args.predict_repeats}
    rec["whole"] = _host_time(lambda: corrupt.predict_split(model, store, split, size, mean, std, names, sev, "both", args.seed,
                                                            args.batch), args.predict_repeats)
    g = torch.Generator(device=dev).manual_seed(args.seed)
    pair = [torch.rand(args.batch, 3, args.size, args.size, device=dev, generator=g) for _ in range(2)]
    pos = np.arange(args.batch)

    def kernels():
        for n in names:
            for s in sev:
                for m, x in enumerate(pair):
                    corrupt.apply(x, n, s, pos, args.seed, m)
    rec["corruptions_alone"] = _host_time(kernels, args.predict_repeats)
    rec["corruption_share"] = rec["corruptions_alone"]["median_s"] / rec["whole"]["median_s"]
    rec["pairs_per_s_per_pass"] = args.batch * rec["passes"] / rec["whole"]["median_s"]
    return rec


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("corrupt_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(args.seed)
    x = torch.rand(args.batch, 3, args.size, args.size, device=dev, generator=g)
    ids = np.arange(args.batch)
    records = [bench_kernel(args, dev, x, ids, n, s) for n in KERNEL_OF for s in sorted(args.severities)]
    if args.only == "all":
        records.append(bench_predict(args, dev))
    for rec in records:
        print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        kept = []
        if os.path.isfile(args.out):
            kept = [r for r in json.load(open(args.out)) if r.get("what") not in ("kernel", "predict_split")]
        with open(args.out, "w") as f:
            json.dump(kept + records, f, indent=1)
    return records


if __name__ == "__main__":
    main()
