"""Hand-run generator of the label-projector fixtures (tests/golden/mlc_proj_*.npz, mlc_proj_state_dict_shapes.json), produced
by the REFERENCE'S OWN MODULES.

The reference's `src/models/projector.py` (MultiLabelProjector, 2, 3, 4) and the `Model` class of its `tools/mlc_train.py`
(:58-90) are taken out of its source with `ast` AT GENERATION TIME (nothing of them is stored in this repository) and run in
fp64 on CPU, with a stub extractor whose `extract` returns fixed features.  Parameters and features are drawn in fp32 and
widened, so the fp32 engine sees exactly the stored values.  For --mlc-proj v0..v3 (and v2 with --l2-norm) one train-mode
step with dropout 0:
    sa_feats, the eight preds, the pseudo-label loss of mlc_train.py:252-261 on fixed assignments, the gradient of every head
    parameter and of the features, the BatchNorm buffers after the step, and the eval-mode preds taken after it.
The --l2-norm case is forward only: the reference normalises sa_feats in place (mlc_train.py:83-85), which autograd refuses
to differentiate.  Computed in fp64, stored as fp32 (the loss as fp64) to keep the files small.

    python tests/golden/gen_mlc_proj_golden.py [path/to/reference]
"""
import ast
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]
B, IN_DIM, D, HEADS, FF, TEMP = 12, 64, 32, 2, 64, 0.5


def reference_modules():
    ns = {"torch": torch, "nn": nn, "NUM_CLASSES": NUM_CLASSES}
    path = os.path.join(REF, "src", "models", "projector.py")
    exec(compile(open(path).read(), path, "exec"), ns)
    path = os.path.join(REF, "tools", "mlc_train.py")
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Model"]
    assert len(keep) == 1
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns


class StubExtractor(nn.Module):
    def __init__(self, feats):
        super().__init__()
        self.feats = feats

    def extract(self, derm, clinic):
        h = self.feats.shape[1] // 2
        return self.feats[:, :h], self.feats[:, h:]


def projectors(ns, kind, in_dim, d):
    if kind == "v0":
        return nn.Identity()
    cls = {"v1": "MultiLabelProjector", "v2": "MultiLabelProjector2", "v3": "MultiLabelProjector3", "v4": "MultiLabelProjector4"}
    return ns[cls[kind]](in_dim, d, 8)


def case(ns, kind, l2_norm, seed):
    d = IN_DIM if kind == "v0" else D
    torch.manual_seed(seed)
    feats32 = torch.randn(B, IN_DIM)
    model = ns["Model"](None, projectors(ns, kind, IN_DIM, d), d, l2_norm, HEADS, FF, 0.0)
    with torch.no_grad():  # non-trivial BatchNorm affine parameters and running buffers
        for name, t in model.named_parameters():
            if name.startswith("projectors.") and t.dim() == 1:
                t.copy_((1.0 if name.endswith(".weight") else 0.0) + 0.2 * torch.randn(t.shape))
        for name, t in model.named_buffers():
            if name.endswith("running_mean"):
                t.copy_(0.1 * torch.randn(t.shape))
            elif name.endswith("running_var"):
                t.copy_(0.5 + torch.rand(t.shape))
            elif name.endswith("num_batches_tracked"):
                t.fill_(3)
    model = model.double()
    feats = feats32.double().requires_grad_(True)
    model.extractor = StubExtractor(feats)
    init = {k: v.detach().clone().numpy() for k, v in model.state_dict().items() if not k.startswith("extractor")}
    g = torch.Generator().manual_seed(seed + 1)
    targets = torch.stack([torch.randint(0, n, (B,), generator=g) for n in NUM_CLASSES])
    model.train()
    sa_feats, preds = model(None, None)
    crit = nn.CrossEntropyLoss(ignore_index=-100)
    loss = sum(crit(p / TEMP, t) for p, t in zip(preds, targets)) / len(NUM_CLASSES)  # mlc_train.py:252-261
    if not l2_norm:
        loss.backward()
    out = {"feats": feats32.numpy(), "targets": targets.numpy(), "temperature": np.float64(TEMP), "l2_norm": np.int64(l2_norm),
           "sa_feats": sa_feats.detach().numpy(), "preds": torch.cat([p.detach() for p in preds], 1).numpy(),
           "loss": np.float64(loss.item())}
    if not l2_norm:
        out["grad:feats"] = feats.grad.numpy()
        for name, p in model.named_parameters():
            out["grad:" + name] = p.grad.numpy()
    for k, v in init.items():
        out["init:" + k] = v
    for name, t in model.named_buffers():
        out["after:" + name] = t.detach().clone().numpy()
    model.eval()
    with torch.no_grad():
        _, preds_eval = model(None, None)
    out["preds_eval"] = torch.cat(preds_eval, 1).numpy()
    return {k: (v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v) for k, v in out.items()}


def main():
    ns = reference_modules()
    for kind, l2, seed in (("v0", False, 10), ("v1", False, 11), ("v2", False, 12), ("v3", False, 13), ("v2", True, 14)):
        out = case(ns, kind, l2, seed)
        name = f"mlc_proj_{kind}{'_l2' if l2 else ''}_f64.npz"
        np.savez_compressed(os.path.join(HERE, name), **out)
        print("wrote", name, "loss", float(out["loss"]))
    shapes = {}
    for kind in ("v1", "v2", "v3", "v4"):
        for in_dim, d in ((IN_DIM, D), (4096, 512)):
            sd = projectors(ns, kind, in_dim, d).state_dict()
            shapes[f"{kind}_{in_dim}_{d}"] = [[k, list(v.shape)] for k, v in sd.items()]
    with open(os.path.join(HERE, "mlc_proj_state_dict_shapes.json"), "w") as f:
        json.dump(shapes, f)
    print("wrote mlc_proj_state_dict_shapes.json")


if __name__ == "__main__":
    main()
