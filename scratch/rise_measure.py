"""rise cost (profiles/rise_measure.json): 8 pairs at 224^2, ResNet-50 Baseline, bf16, 4000 masks, 7 cells, joint, against the
same kind of maps through stock torch on the same engine (torch.rand grids, F.interpolate(mode="bilinear"), crop at a random shift,
multiply, model([derm, clinic]) per chunk, one einsum for the weighted sum -- the parent commit has no such path; its masks are
other random numbers, so the maps are compared by their statistics only); the time by chunk; and the three kernels alone:
sm3_rise_table, sm3_rise_compose's bytes per second, sm3_rise_accumulate at 64 and 16 rows (a build with
-DSM3_RISE_ROW_TILE=4 or 16, loaded through SM3_LIBRARY, times the other row tiles).
python scratch/rise_measure.py [reps] [out.json]; reps = 0: two rise calls only (for rocprofv3); "accumulate": that kernel alone."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # scratch/ -> repository root
sys.path[:0] = [ROOT, os.path.join(ROOT, "skin-sm3_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from oracle import procedural  # noqa: E402
from src.models.baseline import Baseline  # noqa: E402
from sm3hip import ops  # noqa: E402
from sm3hip.rise import rise  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1] != "accumulate" else 10
N, S, M, CELLS, P, T = 8, 224, 4000, 7, 0.5, 8
dev = torch.device("cuda", 0)


def timed(fn, warm=2, reps=reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "reps": reps}


def accumulate_times():
    """sm3_rise_accumulate alone, 4000 masks of 224^2 at 64 and 16 rows (8 labels x 8 and 2 pairs)."""
    tab = torch.empty(M, ops.RISE_ROW_WORDS, dtype=torch.int32, device=dev)
    ops.rise_table(tab, 0, 0, S, S, CELLS, P, 1)
    gen, res = torch.Generator(device=dev).manual_seed(2), {}
    for pairs in (N, 2):
        w = torch.rand(M, pairs * T, device=dev, generator=gen)
        acc = torch.empty(pairs, T, 2, S, S, device=dev)
        r = timed(lambda: ops.rise_accumulate(tab, w, acc[:, :, 0], CELLS, P))
        r["separately_rounded_flop_per_s"] = 2.0 * pairs * T * S * S * M / (r["median_ms"] * 1e-3)
        res[f"rows {pairs * T}"] = r
    return res


if len(sys.argv) > 1 and sys.argv[1] == "accumulate":  # the row-tile variants: SM3_LIBRARY=<a build with another tile>
    print(json.dumps({"library": os.environ.get("SM3_LIBRARY", "default"), "rise_accumulate": accumulate_times()}, indent=1))
    sys.exit(0)

state = procedural.make_state_dict(procedural.baseline_spec(), seed=1)
m = Baseline("resnet50", None)
m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
for b in (m.derm_backbone, m.clinic_backbone):
    b.sm3_dtype = torch.bfloat16
m.to(dev).eval()
for p in m.parameters():
    p.requires_grad_(False)
g = torch.Generator(device=dev).manual_seed(0)
derm = torch.randn(N, 3, S, S, device=dev, generator=g)
clinic = torch.randn(N, 3, S, S, device=dev, generator=g)
run = lambda **kw: rise(m, derm, clinic, masks=M, cells=CELLS, p=P, seed=1, **kw)
if reps == 0:
    run(), run()
    torch.cuda.synchronize()
    sys.exit(0)
first = run()
CHUNK, tc = first["chunk"], first["target_class"]


def torch_route():
    """RISE as its authors' code makes it, with stock torch ops around the same engine, the chunk of the call above."""
    with torch.no_grad():
        cell = -(-S // CELLS)
        up = (CELLS + 1) * cell
        gen = torch.Generator(device=dev).manual_seed(1)
        masks = torch.empty(2, M, S, S, device=dev)
        weights = torch.empty(M, N * T, device=dev)
        for i0 in range(0, M, CHUNK):
            c = min(CHUNK, M - i0)
            ins = []
            for mod, x in enumerate((derm, clinic)):
                grid = (torch.rand(c, 1, CELLS, CELLS, device=dev, generator=gen) < P).float()
                big = F.interpolate(grid, size=(up, up), mode="bilinear", align_corners=False)
                oy, ox = [int(v) for v in torch.randint(0, cell, (2,), generator=gen, device=dev)]
                mk = big[:, 0, oy:oy + S, ox:ox + S]
                masks[mod, i0:i0 + c] = mk
                ins.append((mk[:, None, None] * x[None]).reshape(c * N, 3, S, S))
            logits = m(ins)
            for t in range(T):
                pr = torch.softmax(logits[t].double(), 1).gather(1, tc[:, t].repeat(c)[:, None])
                weights[i0:i0 + c, t::T] = pr.view(c, N).float()
        maps = torch.einsum("ir,mihw->rmhw", weights, masks) / (M * P)
        return maps.view(N, T, 2, S, S)


out = {"config": f"Baseline(resnet50 x2), bf16, {N} pairs, {S}x{S}, {M} masks, {CELLS} cells, p {P}, joint, 8 labels, device events "
                 "around each call, 2 warm-up calls", "chunk": CHUNK}
out["rise"] = timed(run)
out["torch_route"] = timed(torch_route)
out["torch_over_rise"] = out["torch_route"]["median_ms"] / out["rise"]["median_ms"]
images = 2 * M * N + 2 * N  # masked images through the encoders per call, and the pair itself
out["rise"]["encoder_images_per_s"] = images / (out["rise"]["median_ms"] * 1e-3)
out["torch_route"]["encoder_images_per_s"] = images / (out["torch_route"]["median_ms"] * 1e-3)
# the planned chunk is capped at faith.MAX_FORWARD_IMAGES = 1024 images per forward (128 masks here)
out["by_chunk_median_ms"] = {str(c): timed(lambda c=c: run(chunk=c), warm=1, reps=max(3, reps // 2))["median_ms"]
                             for c in (32, 64, 128)}
ref = torch_route()
mp = first["maps"]
out["maps"] = {"rise_mean": float(mp.mean()), "rise_min": float(mp.min()), "rise_max": float(mp.max()),
               "torch_mean": float(ref.mean()), "torch_min": float(ref.min()), "torch_max": float(ref.max()),
               "scores_min": float(first["scores"].min()), "scores_max": float(first["scores"].max())}
# the three kernels alone
tab = torch.empty(M, ops.RISE_ROW_WORDS, dtype=torch.int32, device=dev)
out["rise_table_4000"] = timed(lambda: ops.rise_table(tab, 0, 0, S, S, CELLS, P, 1))
c = min(CHUNK, M)
xin = torch.empty(c, N, 3, S, S, device=dev)
zero = torch.zeros(1, 3, S, S, device=dev)
out["rise_compose"] = timed(lambda: ops.rise_compose(derm, zero, tab[:c], xin, CELLS))
moved = 4.0 * (xin.numel() + (c + 7) // 8 * (derm.numel() + 3 * S * S)) + 144.0 * c  # stores; x and the baseline per 8 masks
out["rise_compose"].update(bytes=moved, masks=c, tb_per_s=moved / (out["rise_compose"]["median_ms"] * 1e-3) / 1e12)
out["rise_compose"]["whole_call_ms"] = out["rise_compose"]["median_ms"] * 2 * M / c
out["rise_accumulate"] = accumulate_times()
print(json.dumps(out, indent=1))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
