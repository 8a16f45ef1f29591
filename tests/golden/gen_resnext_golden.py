"""Hand-run generator of the ResNeXt fixtures in this directory (never imported by a test).

Builds the reference's own modules on CPU through ``oracle.ref_stub``, fills them with the procedural weights
(``oracle.procedural.fill_tensor`` over the model's own key / shape list) and writes, in fp64:

    sm3_v32_rx50_b4_s64_f64.npz       one SimCLRSkinV32("resnext50_32x4d") training step (style 0, AdamW) on
                                      ``procedural.make_pair_batch`` images: loss, logits, gradient norms / sums / subsamples,
                                      post-step norms
    rx101_32x8d_feat_b2_s64_f64.npz   pooled features of resnext101_32x8d (fc = Identity) on 2 images, eval and train mode
    rx101_64x4d_feat_b2_s64_f64.npz   ... of resnext101_64x4d
    rx50_state_dict_keys.txt          SimCLRSkinV32("resnext50_32x4d") state_dict keys, in order
    rx50_state_dict_shapes.json       ... and their shapes

    SM3_REFERENCE=<reference checkout> python tests/golden/gen_resnext_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import procedural, ref_stub  # noqa: E402
from gen_resnet18_golden import REF, SEED, procedural_state, sm3_step  # noqa: E402

FEAT_BATCH, FEAT_SEED = 2, 7


def features(resnet_mod, arch, tag):
    out = {"meta": np.array([FEAT_BATCH, 64, FEAT_SEED], dtype=np.int64)}
    x_np, _ = procedural.make_pair_batch(FEAT_BATCH, 64, FEAT_SEED)
    x = torch.from_numpy(x_np[0]).double()
    for mode in ("eval", "train"):
        torch.manual_seed(0)
        model = resnet_mod.__dict__[arch](weights=None)
        model.load_state_dict(procedural_state(model, SEED), strict=True)
        model.fc = torch.nn.Identity()
        model = model.double().train(mode == "train")
        with torch.no_grad():
            out["feat_" + mode] = model(x).numpy()
    path = os.path.join(HERE, f"{tag}_feat_b2_s64_f64.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


def main():
    if not REF:
        raise SystemExit("set SM3_REFERENCE to the reference checkout")
    ref_stub.install()
    sys.path.insert(0, REF)
    from src.models import resnet
    from src.models.simclr import SimCLRSkinV32

    sd = sm3_step(SimCLRSkinV32, "resnext50_32x4d", "rx50")
    with open(os.path.join(HERE, "rx50_state_dict_keys.txt"), "w") as f:
        f.write("\n".join(sd.keys()) + "\n")
    with open(os.path.join(HERE, "rx50_state_dict_shapes.json"), "w") as f:
        json.dump([[k, list(v.shape)] for k, v in sd.items()], f)
    features(resnet, "resnext101_32x8d", "rx101_32x8d")
    features(resnet, "resnext101_64x4d", "rx101_64x4d")


if __name__ == "__main__":
    main()
