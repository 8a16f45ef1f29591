"""grad_cam cost (profiles/cam_measure.json): 64 pairs at 224^2, ResNet-50 Baseline, bf16, layer4 and layer3, against one
eval forward.  python scratch/cam_measure.py [reps] [out.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # scratch/ -> repository root
sys.path[:0] = [ROOT, os.path.join(ROOT, "skin-sm3_amd")]
import torch  # noqa: E402
from oracle import procedural  # noqa: E402
from src.models.baseline import Baseline  # noqa: E402
from sm3hip.cam import grad_cam  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
dev = torch.device("cuda", 0)
state = procedural.make_state_dict(procedural.baseline_spec(), seed=1)
m = Baseline("resnet50", None)
m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
for b in (m.derm_backbone, m.clinic_backbone):
    b.sm3_dtype = torch.bfloat16
m.to(dev).eval()
g = torch.Generator(device=dev).manual_seed(0)
derm = torch.randn(64, 3, 224, 224, device=dev, generator=g)
clinic = torch.randn(64, 3, 224, 224, device=dev, generator=g)


def timed(fn):
    for _ in range(3):
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


def fwd():
    with torch.no_grad():
        m([derm, clinic])


out = {"config": "Baseline(resnet50 x2), bf16, 64 pairs, 224x224, target=pred, device events around each call",
       "eval_forward": timed(fwd)}
for layer in ("layer4", "layer3"):
    out[f"grad_cam_{layer}"] = timed(lambda: grad_cam(m, derm, clinic, layer=layer))
for layer in ("layer4", "layer3"):
    out[f"grad_cam_{layer}"]["over_forward"] = out[f"grad_cam_{layer}"]["median_ms"] / out["eval_forward"]["median_ms"]
print(json.dumps(out, indent=1))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f, indent=1)
