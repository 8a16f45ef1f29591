"""deletion_insertion cost (profiles/faith_measure.json): 8 pairs at 224^2, ResNet-50 Baseline, bf16, 32 curve steps, both curves,
Grad-CAM maps, against the same curves through stock torch on the same engine (torch.argsort(stable=True) for the ranks,
torch.where for the masked inputs, model([derm, clinic]) per chunk -- the parent commit has no such path); beside it the two
kernels alone: sm3_faith_rank on the call's 128 maps against torch.argsort, sm3_faith_compose's bytes per second.
python scratch/faith_measure.py [reps] [out.json]; reps = 0: two deletion_insertion calls only (for rocprofv3)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # scratch/ -> repository root
sys.path[:0] = [ROOT, os.path.join(ROOT, "skin-sm3_amd")]
import torch  # noqa: E402
from oracle import procedural  # noqa: E402
from src.models.baseline import Baseline  # noqa: E402
from sm3hip import ops  # noqa: E402
from sm3hip.cam import grad_cam  # noqa: E402
from sm3hip.faith import auc, counts, deletion_insertion  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
N, S, STEPS, T = 8, 224, 32, 8
dev = torch.device("cuda", 0)
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
cam = grad_cam(m, derm, clinic)
maps, tc = cam["maps"], cam["target_class"]
run = lambda: deletion_insertion(m, derm, clinic, maps, target=tc, steps=STEPS)
if reps == 0:
    run(), run()
    torch.cuda.synchronize()
    sys.exit(0)
first = run()
CHUNK = first["chunk"]


def torch_route():
    """The same curves with stock torch ops around the same engine, the chunk of the call above."""
    with torch.no_grad():
        order = torch.argsort(-maps.view(N, T, 2, -1), dim=-1, stable=True)
        ranks = torch.empty_like(order)
        ranks.scatter_(-1, order, torch.arange(S * S, device=dev).expand_as(order))
        ranks = ranks.view(N, T, 2, S, S)
        ck = counts(S * S, STEPS)
        xs = (derm, clinic)
        pick = lambda lg, t, rows: torch.softmax(lg.double(), 1).gather(1, tc[:, t].repeat(rows // N)[:, None])[:, 0]
        at_x, at_b = m([derm, clinic]), m([torch.zeros_like(derm), torch.zeros_like(clinic)])
        ends = [torch.stack([pick(o, t, N) for t, o in enumerate(lg)], 1) for lg in (at_x, at_b)]
        out = {}
        for name, invert in (("deletion", False), ("insertion", True)):
            curve = torch.empty(N, T, STEPS + 1, dtype=torch.float64, device=dev)
            curve[..., 0], curve[..., STEPS] = ends[int(invert)], ends[1 - int(invert)]
            for k0 in range(1, STEPS, CHUNK):
                c = min(CHUNK, STEPS - k0)
                cks = torch.tensor(ck[k0:k0 + c], device=dev).view(c, 1, 1, 1, 1, 1)
                ins = []
                for mod in range(2):
                    sel = ((ranks[:, :, mod].permute(1, 0, 2, 3)[None, :, :, None] < cks) != invert)  # [c, T, N, 1, H, W]
                    ins.append(torch.where(sel, torch.zeros((), device=dev), xs[mod][None, None]).reshape(c * T * N, 3, S, S))
                logits = m(ins)
                for t in range(T):
                    lg = logits[t].view(c, T, N, -1)[:, t].reshape(c * N, -1)
                    curve[:, t, k0:k0 + c] = pick(lg, t, c * N).view(c, N).t()
            out[name], out[name + "_auc"] = curve, auc(curve)
        return out, ranks


def timed(fn, warm=2):
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


out = {"config": f"Baseline(resnet50 x2), bf16, {N} pairs, {S}x{S}, {STEPS} curve steps, both curves, joint, 8 labels, Grad-CAM "
                 "layer4 maps, device events around each call, 2 warm-up calls", "chunk": CHUNK}
out["deletion_insertion"] = timed(run)
out["torch_route"] = timed(torch_route)
out["torch_over_deletion_insertion"] = out["torch_route"]["median_ms"] / out["deletion_insertion"]["median_ms"]
# the planned chunk is capped at faith.MAX_FORWARD_IMAGES = 1024 images per forward (16 steps here); below and above the cap:
out["by_chunk_median_ms"] = {str(c): timed(lambda c=c: deletion_insertion(m, derm, clinic, maps, target=tc, steps=STEPS, chunk=c))
                             ["median_ms"] for c in (4, 8, 16, 31)}
images = 2 * 2 * (STEPS - 1) * T * N + 4 * N  # perturbed images through the encoders per call, and the two end states
out["deletion_insertion"]["encoder_images_per_s"] = images / (out["deletion_insertion"]["median_ms"] * 1e-3)
out["torch_route"]["encoder_images_per_s"] = (2 * 2 * (STEPS - 1) * T * N + 4 * N) / (out["torch_route"]["median_ms"] * 1e-3)
ref, ref_ranks = torch_route()
out["ranks_equal"] = bool(torch.equal(first["ranks"].long(), ref_ranks))
out["curves_max_abs_diff"] = max(float((first[k] - ref[k]).abs().max()) for k in ("deletion", "insertion"))
out["mean_deletion_auc"], out["mean_insertion_auc"] = float(first["deletion_auc"].mean()), float(first["insertion_auc"].mean())
# the two kernels alone
flat = maps.contiguous().view(N * T * 2, S * S)
rk = torch.empty(flat.shape, dtype=torch.int32, device=dev)
out["faith_rank_128_maps"] = timed(lambda: ops.faith_rank(flat, rk))
out["torch_argsort_128_maps"] = timed(lambda: torch.argsort(-flat, dim=-1, stable=True))
c = min(CHUNK, STEPS - 1)
xin = torch.empty(c, T, N, 3, S, S, device=dev)
zero = torch.zeros(1, 3, S, S, device=dev)
out["faith_compose"] = timed(lambda: ops.faith_compose(derm, zero, first["ranks"][:, :, 0], xin, 1, STEPS, False))
moved = 4.0 * (xin.numel() + T * N * S * S + N * 3 * S * S + 3 * S * S)  # stores; the ranks, the images and the baseline once
out["faith_compose"]["bytes"] = moved
out["faith_compose"]["steps"] = c
out["faith_compose"]["tb_per_s"] = moved / (out["faith_compose"]["median_ms"] * 1e-3) / 1e12
print(json.dumps(out, indent=1))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
