"""derm7pt-size measurement (profiles/derm7pt_measure.json): store build, real-data vs synthetic --gpu-augment backbone_train
steps (ResNet-50, B=256, bf16), alternated in one process.  python scratch/derm7pt_measure.py [out.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "skin-sm3_amd")]
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402


def make_tree(root, n_train=413, n_val=10, n_test=10, seed=0):
    g = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    n = n_train + n_val + n_test
    rows = []
    yy, xx = np.mgrid[0:512, 0:768]
    for i in range(n):
        for kind, (h, w) in (("d", (512, 768)), ("c", (int(g.integers(400, 900)), int(g.integers(500, 1100))))):
            ph = g.uniform(0, 6, 3)
            base = np.stack([128 + 90 * np.sin(xx[:h, :w] / (20 + 5 * c) + ph[c]) * np.cos(yy[:h, :w] / 17.0) for c in range(3)], -1)
            if h > 512 or w > 768:
                base = np.asarray(Image.fromarray(base.astype(np.uint8)).resize((w, h)))
            img = np.clip(base + g.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(root, "images", f"{kind}{i:04d}.jpg"), quality=90)
        rows.append({"diagnosis": "nevus", "pigment_network": "absent", "blue_whitish_veil": "absent",
                     "vascular_structures": "absent", "pigmentation": "absent", "streaks": "absent",
                     "dots_and_globules": "absent", "regression_structures": "absent", "elevation": "flat", "sex": "male",
                     "location": "back", "derm": f"d{i:04d}.jpg", "clinic": f"c{i:04d}.jpg"})
    pd.DataFrame(rows).to_csv(os.path.join(root, "meta.csv"), index=False)
    for name, idx in (("train", range(n_train)), ("valid", range(n_train, n_train + n_val)), ("test", range(n_train + n_val, n))):
        pd.DataFrame({"indexes": list(idx)}).to_csv(os.path.join(root, f"{name}_indexes.csv"), index=False)


def main():
    import types
    from sm3hip.augment import SimCLRAugment, chain
    from sm3hip.imagestore import ImageStore
    from sm3hip.trainer import SM3Trainer
    from src.models.simclr import SimCLRSkinV32
    from src.utils.data.datasets import SevenPCBaseDataset
    from src.utils.data.sampler import train_batches
    res = {}
    root = "/tmp/derm7pt_bench"
    t0 = time.time()
    make_tree(root)
    res["tree_gen_s"] = time.time() - t0
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    args = types.SimpleNamespace(data_path=root, workers=16)
    ds = SevenPCBaseDataset(args, None, "train")
    store = ImageStore({"train": ds}, dev, workers=16)
    res["store_images"] = len(store)
    res["store_mib"] = store.arena.numel() / 2 ** 20
    res["store_build_s"] = store.build_seconds
    store2 = ImageStore({"train": ds}, dev, workers=16)   # second build: page cache warm
    res["store_build_warm_s"] = store2.build_seconds
    del store2
    B, S = 256, 224
    mean, std = [0.7833, 0.6712, 0.6026], [0.2139, 0.2472, 0.2571]
    model = SimCLRSkinV32("resnet50", None, 128, 0.1)
    model.sm3_dtype = torch.bfloat16
    model = model.to(dev)
    trainer = SM3Trainer(model, lr=1e-6, weight_decay=0.05, eps=1e-5, style=0)
    aug = chain("backbone_train", (S, S), mean, std)
    syn = SimCLRAugment((S, S), mean, std)
    split = store.splits["train"]
    order = torch.cat(train_batches(len(split), 1, 0, 0, len(split)))
    gen = torch.Generator(device=dev).manual_seed(1)
    ag, sg = torch.Generator().manual_seed(2), torch.Generator().manual_seed(3)
    state = {"k": 0}

    def real_views():
        k = state["k"]
        sel = torch.cat([order, order])[k:k + B]
        state["k"] = (k + B) % len(order)
        return store.augment(aug, split.derm_ids[sel], ag, 2), store.augment(aug, split.clinic_ids[sel], ag, 2)

    def syn_views():
        src_hw = (2 * S + 14, 3 * S + 46)
        d = torch.randint(0, 256, (B,) + src_hw + (3,), device=dev, generator=gen, dtype=torch.uint8)
        c = torch.randint(0, 256, (B,) + src_hw + (3,), device=dev, generator=gen, dtype=torch.uint8)
        return syn(d, sg), syn(c, sg)

    def block(fn, steps, train=True):
        torch.cuda.synchronize()
        t = time.time()
        for _ in range(steps):
            d, c = fn()
            if train:
                trainer.step(d, c)
        torch.cuda.synchronize()
        return (time.time() - t) / steps

    for fn in (real_views, syn_views):
        block(fn, 3)
    rounds = {"real": [], "synthetic": [], "real_aug_only": [], "synthetic_aug_only": []}
    for _ in range(3):
        rounds["real"].append(block(real_views, 10))
        rounds["synthetic"].append(block(syn_views, 10))
        rounds["real_aug_only"].append(block(real_views, 10, train=False))
        rounds["synthetic_aug_only"].append(block(syn_views, 10, train=False))
    # host parameter draws alone (4 view batches per step)
    hs, ws = store.img_h[split.derm_ids[:B].long()], store.img_w[split.derm_ids[:B].long()]
    t = time.time()
    for _ in range(4):
        aug.sample_ragged(hs, ws, ag)
    res["host_draw_ragged_ms_per_step"] = (time.time() - t) * 1e3
    t = time.time()
    for _ in range(4):
        syn.sample(B, 462, 718, sg)
    res["host_draw_fixed_ms_per_step"] = (time.time() - t) * 1e3
    for k, v in rounds.items():
        res[f"{k}_ms_per_step"] = [round(x * 1e3, 2) for x in v]
        res[f"{k}_pairs_per_s"] = round(B / min(v), 1)
    res["real_vs_synthetic"] = round(min(rounds["synthetic"]) / min(rounds["real"]), 4)
    print(json.dumps(res), flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else "derm7pt_measure.json"
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
