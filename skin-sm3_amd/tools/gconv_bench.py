"""Per-shape timing of the grouped 3x3 convolution kernels (csrc/gconv.hip) at the conv2 shapes of a ResNeXt.

For every conv2 of the chosen architecture at 224 x 224 (one row per distinct (width, groups, map, stride)), times the forward
(with BatchNorm partial rows), the data gradient and the weight gradient on `--images` images with HIP events, and prints
the time and the algorithmic bytes / time: the forward reads x and the bank and writes y; the data gradient reads dy and the
bank and writes dx; the weight gradient reads x and dy and writes its slabs.

    python skin-sm3_amd/tools/gconv_bench.py -a resnext50_32x4d --images 512 --dtype bf16
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

ARCHS = {"resnext50_32x4d": (32, 4), "resnext101_32x8d": (32, 8), "resnext101_64x4d": (64, 4)}


def shapes(groups, wpg):
    out, h = [], 56
    for li, planes in enumerate((64, 128, 256, 512)):
        width = int(planes * wpg / 64) * groups
        if li:
            out.append((width, groups, h, 2))
            h //= 2
        out.append((width, groups, h, 1))
    return out


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-a", "--arch", default="resnext50_32x4d", choices=list(ARCHS))
    ap.add_argument("--images", type=int, default=512, help="images per launch (256 pairs = 512 with both views)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    from sm3hip import ops
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[args.dtype]
    code, sz = ops.dtype_code(dt), torch.finfo(dt).bits // 8
    dev = torch.device("cuda", 0)
    N = args.images
    print(f"{args.arch}, {args.dtype}, {N} images per launch; time in us, algorithmic TB/s")
    print(f"{'C':>5} {'G':>3} {'H':>3} {'s':>2} | {'fwd us':>9} {'TB/s':>6} | {'dgrad us':>9} {'TB/s':>6} | {'wgrad us':>9} {'TB/s':>6}")
    for C, G, H, s in shapes(*ARCHS[args.arch]):
        Ho = (H - 1) // s + 1
        cg = C // G
        n = C * 9 * cg
        x = torch.randn(N * H * H, C, device=dev).to(dt)
        dy = torch.randn(N * Ho * Ho, C, device=dev).to(dt)
        master = torch.randn(n, device=dev) * 0.05
        wf, wd = torch.empty(n, dtype=dt, device=dev), torch.empty(n, dtype=dt, device=dev)
        ops.gconv_weight_prep(code, master, C, G, wf, wd)
        y = torch.empty(N * Ho * Ho, C, dtype=dt, device=dev)
        dx = torch.empty_like(x)
        part = torch.empty((N * Ho * Ho + 127) // 128 * 2 * C, device=dev)
        dw = torch.zeros(n, device=dev)
        cap = ops.wgrad_det_cap(n)
        slabs = torch.empty(cap * n, device=dev)
        tf = timed(lambda: ops.gconv_fwd(code, x, wf, y, part, N, H, H, C, G, s), args.reps)
        td = timed(lambda: ops.gconv_dgrad(code, dy, wd, dx, N, H, H, C, G, s), args.reps)
        tw = timed(lambda: ops.gconv_wgrad_det(code, x, dy, dw, slabs, cap, N, H, H, C, G, s), args.reps)
        bf = sz * (x.numel() + y.numel() + n)
        bd = sz * (dy.numel() + dx.numel() + n)
        bw = sz * (x.numel() + dy.numel()) + 4 * n
        print(f"{C:>5} {G:>3} {H:>3} {s:>2} | {tf * 1e6:>9.1f} {bf / tf / 1e12:>6.2f} | {td * 1e6:>9.1f} {bd / td / 1e12:>6.2f} | "
              f"{tw * 1e6:>9.1f} {bw / tw / 1e12:>6.2f}", flush=True)
        del x, dy, y, dx, part, slabs


if __name__ == "__main__":
    main()
