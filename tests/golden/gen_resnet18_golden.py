"""Hand-run generator of the ResNet-18 fixtures in this directory (never imported by a test).

Builds the reference's own ``SimCLRSkinV32("resnet18", None, 128, 0.1)`` on CPU through ``oracle.ref_stub``, fills it
with the procedural weights (``oracle.procedural.fill_tensor`` over the model's own key / shape list), runs one training
step the way ``tools/backbone_train.py`` composes it (style 0, fp64, AdamW) on ``procedural.make_pair_batch`` images
and writes

    sm3_v32_r18_b4_s64_f64.npz       loss, logits, gradient norms / sums / subsamples, post-step norms
    sm3_v32_r34_b4_s64_f64.npz       the same step of SimCLRSkinV32("resnet34")
    baseline_r18_b4_s64_f64.npz      Baseline("resnet18"): eval-mode logits, weighted-CE loss, head gradients (linear probe)
    r18_state_dict_keys.txt          SimCLRSkinV32("resnet18") state_dict keys, in order
    r18_state_dict_shapes.json       ... and their shapes
    r18_baseline_state_dict_keys.txt Baseline("resnet18") state_dict keys, in order

    SM3_REFERENCE=<reference checkout> python tests/golden/gen_resnet18_golden.py
"""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import procedural, ref_stub  # noqa: E402

REF = os.environ.get("SM3_REFERENCE")
BATCH, SIZE, SEED, STYLE, LR = 4, 64, 5, 0, 1e-3


def subsample(t, n=256):
    flat = t.detach().reshape(-1)
    step = max(1, flat.numel() // n)
    return flat[::step][:n].double().numpy()


def procedural_state(model, seed):
    return OrderedDict((k, torch.from_numpy(np.asarray(procedural.fill_tensor(k, tuple(v.shape), seed))))
                       for k, v in model.state_dict().items())


GRAD_SUB = ("derm_backbone.encoder.conv1.weight", "derm_backbone.encoder.layer1.0.conv1.weight",
            "derm_backbone.encoder.layer2.0.conv1.weight", "derm_backbone.encoder.layer2.0.downsample.0.weight",
            "clinic_backbone.encoder.layer3.1.conv2.weight", "clinic_backbone.encoder.layer4.0.conv1.weight",
            "derm_backbone.projector.0.weight", "cross_proj.1.3.weight")


def sm3_step(SimCLRSkinV32, arch, tag):
    torch.manual_seed(0)
    model = SimCLRSkinV32(arch, None, 128, 0.1)
    model.load_state_dict(procedural_state(model, SEED), strict=True)
    model = model.double().train()
    derm_np, clinic_np = procedural.make_pair_batch(BATCH, SIZE, SEED)
    derm = [torch.from_numpy(a).double() for a in derm_np]
    clinic = [torch.from_numpy(a).double() for a in clinic_np]
    crit = torch.nn.CrossEntropyLoss()
    opt = torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=5e-2, eps=1e-5)
    outputs = model(derm, clinic, STYLE)
    cross = sum(0.5 * crit(*o) for o in outputs[2])
    loss = crit(*outputs[0]) + crit(*outputs[1]) + cross
    opt.zero_grad(set_to_none=True)
    loss.backward()
    params = OrderedDict(model.named_parameters())
    out = {
        "meta": np.array([BATCH, SIZE, SEED, STYLE], dtype=np.int64),
        "lr": np.array(LR),
        "loss": np.array(loss.item()),
        "derm_logits": outputs[0][0].detach().numpy(),
        "clinic_logits": outputs[1][0].detach().numpy(),
        "grad_norm": np.array([p.grad.norm().item() for p in params.values()]),
        "grad_sum": np.array([p.grad.sum().item() for p in params.values()]),
    }
    for i, o in enumerate(outputs[2]):
        out[f"cross_logits_{i}"] = o[0].detach().numpy()
    for k in GRAD_SUB:
        if k in params:
            out["grad_sub." + k] = subsample(params[k].grad)
    opt.step()
    sd = model.state_dict()
    out["post_param_norm"] = np.array([sd[k].norm().item() for k in params])
    bn_keys = [k for k in sd if k.endswith(("running_mean", "running_var"))]
    out["post_buf_norm"] = np.array([sd[k].norm().item() for k in bn_keys])
    path = os.path.join(HERE, f"sm3_v32_{tag}_b4_s64_f64.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: loss={loss.item():.8f} ({os.path.getsize(path) / 1024:.0f} KiB)")
    return sd


def baseline_probe(Baseline):
    """--finetune fc: frozen eval-mode encoders, one weighted-CE backward through the eight heads."""
    torch.manual_seed(0)
    model = Baseline("resnet18", None)
    model.load_state_dict(procedural_state(model, SEED), strict=True)
    model = model.double().eval()
    for p in list(model.derm_backbone.parameters()) + list(model.clinic_backbone.parameters()):
        p.requires_grad = False
    derm_np, clinic_np = procedural.make_pair_batch(BATCH, SIZE, SEED)
    derm, clinic = torch.from_numpy(derm_np[0]).double(), torch.from_numpy(clinic_np[0]).double()
    r = np.random.RandomState(SEED)
    labels = torch.from_numpy(np.stack([r.randint(0, n, size=BATCH) for n in (5, 3, 2, 3, 3, 3, 3, 2)], axis=1)).long()
    crit = torch.nn.CrossEntropyLoss()
    outputs = model([derm, clinic])
    loss = sum(crit(o, labels[:, i]) for i, o in enumerate(outputs)) / 8
    loss.backward()
    out = {"meta": np.array([BATCH, SIZE, SEED], dtype=np.int64), "labels": labels.numpy(), "loss": np.array(loss.item())}
    for i, o in enumerate(outputs):
        out[f"logits_{i}"] = o.detach().numpy()
        out[f"grad_w_{i}"] = model.classifier[i].weight.grad.numpy()
        out[f"grad_b_{i}"] = model.classifier[i].bias.grad.numpy()
    path = os.path.join(HERE, "baseline_r18_b4_s64_f64.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: loss={loss.item():.8f} ({os.path.getsize(path) / 1024:.0f} KiB)")
    return model


def main():
    if not REF:
        raise SystemExit("set SM3_REFERENCE to the reference checkout")
    ref_stub.install()
    sys.path.insert(0, REF)
    from src.models.baseline import Baseline
    from src.models.simclr import SimCLRSkinV32

    sd = sm3_step(SimCLRSkinV32, "resnet18", "r18")
    sm3_step(SimCLRSkinV32, "resnet34", "r34")
    probe = baseline_probe(Baseline)
    with open(os.path.join(HERE, "r18_state_dict_keys.txt"), "w") as f:
        f.write("\n".join(sd.keys()) + "\n")
    with open(os.path.join(HERE, "r18_state_dict_shapes.json"), "w") as f:
        json.dump([[k, list(v.shape)] for k, v in sd.items()], f)
    with open(os.path.join(HERE, "r18_baseline_state_dict_keys.txt"), "w") as f:
        f.write("\n".join(probe.state_dict().keys()) + "\n")


if __name__ == "__main__":
    main()
