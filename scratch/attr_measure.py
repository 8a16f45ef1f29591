"""integrated_gradients cost (profiles/attr_measure.json): 8 pairs at 224^2, ResNet-50 Baseline, bf16, 32 steps, against the same
32 x 8 label gradients through the public autograd route (x.requires_grad_(), model([derm, clinic]), one forward and backward
per label and path point, as tools/backbone_saliency.py takes them), and smooth_grad at 16 samples.
python scratch/attr_measure.py [reps] [out.json]; reps = 0: two integrated_gradients and two smooth_grad calls only (for rocprofv3)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # scratch/ -> repository root
sys.path[:0] = [ROOT, os.path.join(ROOT, "skin-sm3_amd")]
import torch  # noqa: E402
from oracle import procedural  # noqa: E402
from src.models.baseline import Baseline  # noqa: E402
from sm3hip.attr import integrated_gradients, smooth_grad  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
N, S, STEPS, SAMPLES = 8, 224, 32, 16
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
with torch.no_grad():
    tc = torch.stack([o.argmax(dim=1) for o in m([derm, clinic])], dim=1)


def autograd_route():
    """The same 32 x 8 x 2 gradients with what the parent commit offers: the mean gradient over the path per label."""
    acc = [torch.zeros(8, *derm.shape, device=dev), torch.zeros(8, *clinic.shape, device=dev)]
    for k in range(STEPS):
        a = (k + 0.5) / STEPS
        for i in range(8):
            d, c = (a * derm).requires_grad_(), (a * clinic).requires_grad_()
            logit = m([d, c])[i].gather(1, tc[:, i:i + 1]).sum()
            gd, gc = torch.autograd.grad(logit, [d, c])
            acc[0][i] += gd / STEPS
            acc[1][i] += gc / STEPS
    return acc[0] * derm, acc[1] * clinic


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


ig = lambda: integrated_gradients(m, derm, clinic, target=tc, steps=STEPS)
if reps == 0:
    ig(), ig()
    for _ in range(2):
        smooth_grad(m, derm, clinic, target=tc, samples=SAMPLES)
    torch.cuda.synchronize()
    sys.exit(0)
out = {"config": f"Baseline(resnet50 x2), bf16, {N} pairs, {S}x{S}, {STEPS} steps / {SAMPLES} samples, 8 labels, device events "
                 "around each call, 2 warm-up calls"}
first = ig()
out["chunk"] = first["chunk"]
out["integrated_gradients"] = timed(ig)
out["autograd_route"] = timed(autograd_route)
out["smooth_grad"] = timed(lambda: smooth_grad(m, derm, clinic, target=tc, samples=SAMPLES))
out["autograd_over_integrated_gradients"] = out["autograd_route"]["median_ms"] / out["integrated_gradients"]["median_ms"]
per = 2 * N * STEPS * 8  # image gradients per call
out["integrated_gradients"]["image_gradients_per_s"] = per / (out["integrated_gradients"]["median_ms"] * 1e-3)
out["autograd_route"]["image_gradients_per_s"] = per / (out["autograd_route"]["median_ms"] * 1e-3)
# the two routes compute the same attributions (bf16 engine both ways; the autograd route sums in another order)
a, b = first["attributions"], autograd_route()
ref = torch.stack([b[0], b[1]], dim=0).permute(2, 1, 0, 3, 4, 5)
out["routes_rel_diff"] = float((a - ref).norm() / ref.norm())
out["max_abs_delta"] = float(first["delta"].abs().max())
print(json.dumps(out, indent=1))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
