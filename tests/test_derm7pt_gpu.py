"""GPU: derm7pt images from disk -- the ragged crop kernel (sm3_aug_resized_crop_ragged) against the fixed-size one and
against PIL, the device image store against PIL's decode, and the four tools end to end on a small derm7pt-shaped tree."""
import importlib.util
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = os.path.join(ROOT, "tests", "golden", "derm7pt_meta")
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
DEV = "cuda:0"


def _img(g, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin(xx / 9.0 + c) * np.cos(yy / 7.0 - c) for c in range(3)], -1)
    return np.clip(base + g.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def _pack(images):
    """host int64 offsets / int32 sizes and the device arena of a list of [h, w, 3] uint8 arrays"""
    h = torch.tensor([a.shape[0] for a in images], dtype=torch.int32)
    w = torch.tensor([a.shape[1] for a in images], dtype=torch.int32)
    n = h.long() * w.long() * 3
    off = torch.cumsum(n, 0) - n
    arena = torch.from_numpy(np.concatenate([a.reshape(-1) for a in images])).to(DEV)
    return arena, off, h, w


@pytest.mark.parametrize("size", [(64, 64), (48, 80)])
def test_ragged_crop_equals_the_fixed_kernel_bit_for_bit(size):
    from sm3hip import _lib, ops
    from sm3hip.augment import SimCLRAugment
    g = np.random.default_rng(3)
    B, Hs, Ws = 70, 97, 113                  # > one launch chunk of 64 samples
    src = np.stack([_img(g, Hs, Ws) for _ in range(B)])
    aug = SimCLRAugment(size, [0.0] * 3, [1.0] * 3, scale=(0.05, 1.0))   # small boxes: up-scaling, large: down-scaling
    p = aug.sample(B, Hs, Ws, torch.Generator().manual_seed(5))
    H, W = size
    assert bool((p.box[:, 2] < H).any()) and bool((p.box[:, 2] > H).any()) and bool(p.flip.any()) and not bool(p.flip.all())
    lib, st = _lib.load(), ops._stream()
    dsrc = torch.from_numpy(src).to(DEV)
    box, flip = p.box.to(DEV), p.flip.to(DEV)
    want = torch.empty(B, 3, H, W, device=DEV)
    _lib.check(lib.sm3_aug_resized_crop(ops._ptr(dsrc), B, Hs, Ws, ops._ptr(box), ops._ptr(flip), ops._ptr(want), H, W, st), "")
    arena, off, hh, ww = _pack(list(src))
    idx = torch.arange(B, dtype=torch.int32)
    got = torch.empty(B, 3, H, W, device=DEV)
    _lib.check(lib.sm3_aug_resized_crop_ragged(ops._ptr(arena), arena.numel(), off.data_ptr(), hh.data_ptr(), ww.data_ptr(),
                                               B, idx.data_ptr(), p.box.data_ptr(), p.flip.data_ptr(), B, ops._ptr(got), H, W,
                                               st), "")
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # a permuted index list reads the permuted images
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(torch.int32)
    box_p, flip_p = p.box[perm.long()].contiguous(), p.flip[perm.long()].contiguous()
    got_p = torch.empty_like(got)
    _lib.check(lib.sm3_aug_resized_crop_ragged(ops._ptr(arena), arena.numel(), off.data_ptr(), hh.data_ptr(), ww.data_ptr(),
                                               B, perm.data_ptr(), box_p.data_ptr(), flip_p.data_ptr(), B, ops._ptr(got_p), H,
                                               W, st), "")
    torch.cuda.synchronize()
    assert torch.equal(got_p, want[perm.long().to(DEV)])


def test_ragged_crop_rejects_boxes_outside_their_own_image():
    from sm3hip import _lib, ops
    g = np.random.default_rng(0)
    arena, off, hh, ww = _pack([_img(g, 60, 80), _img(g, 90, 70)])
    lib = _lib.load()
    out = torch.empty(2, 3, 16, 16, device=DEV)
    idx = torch.tensor([1, 0], dtype=torch.int32)
    flip = torch.zeros(2, dtype=torch.uint8)
    call = lambda box, index=idx: lib.sm3_aug_resized_crop_ragged(
        ops._ptr(arena), arena.numel(), off.data_ptr(), hh.data_ptr(), ww.data_ptr(), 2, index.data_ptr(), box.data_ptr(),
        flip.data_ptr(), 2, ops._ptr(out), 16, 16, ops._stream())
    assert call(torch.tensor([[0, 0, 90, 70], [0, 0, 60, 80]], dtype=torch.int32)) == 0
    assert call(torch.tensor([[0, 0, 60, 80], [0, 0, 90, 70]], dtype=torch.int32)) == -1   # each box against its OWN image
    assert call(torch.tensor([[1, 0, 90, 70], [0, 0, 60, 80]], dtype=torch.int32)) == -1
    assert call(torch.tensor([[0, 0, 90, 70], [0, 0, 60, 80]], dtype=torch.int32), torch.tensor([1, 2], dtype=torch.int32)) == -1
    torch.cuda.synchronize()


def test_ragged_crop_of_mixed_sizes_against_pil():
    from sm3hip.augment import SimCLRAugment
    g = np.random.default_rng(11)
    sizes = [(300, 420), (462, 718), (560, 780), (333, 500), (512, 512), (420, 300)]
    images = [_img(g, h, w) for h, w in sizes]
    arena, off, hh, ww = _pack(images)
    H, W = 224, 224
    aug = SimCLRAugment((H, W), [0.0] * 3, [1.0] * 3, p_jitter=0.0, p_gray=0.0, p_blur=0.0)
    idx = torch.tensor([0, 1, 2, 3, 4, 5, 1, 0], dtype=torch.int32)
    p = aug.sample_ragged(hh[idx.long()], ww[idx.long()], torch.Generator().manual_seed(2))
    got = aug.apply_ragged(arena, off, hh, ww, idx, p).cpu()
    for b in range(len(idx)):
        i, j, h, w = [int(v) for v in p.box[b]]
        pil = Image.fromarray(images[int(idx[b])]).crop((j, i, j + w, i + h)).resize((W, H), Image.BILINEAR)
        if p.flip[b]:
            pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
        diff = np.abs(got[b].permute(1, 2, 0).numpy().astype(np.float64) * 255.0 - np.asarray(pil).astype(np.float64))
        assert diff.max() <= 1.0 and diff.mean() < 0.4, (b, diff.max(), diff.mean())   # tests/test_augment_pil.py's crop bound


def _write_tree(root, n_cases=30, seed=0):
    """A derm7pt-shaped directory: the fixture's metadata (tests/golden/derm7pt_meta) with PNG / JPEG images of mixed sizes,
    derm 120 x 160 and clinic 100..190 on a side, plus one EXIF-rotated JPEG."""
    g = np.random.default_rng(seed)
    meta = pd.read_csv(os.path.join(META, "meta.csv"))
    assert len(meta) == n_cases
    os.makedirs(root / "images", exist_ok=True)
    derm, clinic = [], []
    for i in range(n_cases):
        ext = "png" if i % 2 else "jpg"
        for kind, names, (h, w) in (("d", derm, (120, 160)), ("c", clinic, (int(g.integers(100, 190)), int(g.integers(100, 190))))):
            name = f"Case{i:03d}/{kind}{i:03d}.{ext}"
            os.makedirs(root / "images" / f"Case{i:03d}", exist_ok=True)
            im = Image.fromarray(_img(g, h, w))
            if kind == "c" and i == 2:
                ex = Image.Exif()
                ex[0x0112] = 6
                im.save(root / "images" / name, quality=90, exif=ex)
            else:
                im.save(root / "images" / name, **({"quality": 90} if ext == "jpg" else {}))
            names.append(name)
    meta["derm"], meta["clinic"] = derm, clinic
    meta.to_csv(root / "meta.csv", index=False)
    for f in ("train_indexes.csv", "valid_indexes.csv", "test_indexes.csv"):
        pd.read_csv(os.path.join(META, f)).to_csv(root / f, index=False)
    return root


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return _write_tree(tmp_path_factory.mktemp("derm7pt") / "7PC")


def test_store_holds_pils_decoded_arrays(tree):
    import types
    from sm3hip.imagestore import ImageStore
    from src.utils.data.datasets import SevenPCBaseDataset
    args = types.SimpleNamespace(data_path=str(tree), workers=4)
    ds = {m: SevenPCBaseDataset(args, None, m) for m in ("train", "val", "test")}
    store = ImageStore(ds, torch.device(DEV), workers=4)
    assert len(store) == 2 * sum(len(d) for d in ds.values())
    rotated = 0
    for k, path in enumerate(store.paths):
        with Image.open(path) as im:
            from PIL import ImageOps
            want = np.asarray(ImageOps.exif_transpose(im).convert("RGB"))[25:-25, 25:-25]
            rotated += im.getexif().get(0x0112, 1) == 6
        assert np.array_equal(store.image(k).cpu().numpy(), want), path
    for m in ds:
        sp = store.splits[m]
        assert torch.equal(sp.labels.cpu(), ds[m].labels)
        assert [store.paths[int(i)] for i in sp.derm_ids] == ds[m].derm_data
        assert [store.paths[int(i)] for i in sp.clinic_ids] == ds[m].clinic_data
    assert rotated == 1
    # the mixed sizes really are mixed
    assert len(set(zip(store.img_h.tolist(), store.img_w.tolist()))) > 5


def _tool(name):
    spec = importlib.util.spec_from_file_location("sm3_derm_gpu_" + name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


DATA = lambda tree: ["--data-name", "SevenPCBaseDataset", "--data-path", str(tree), "-j", "4",
                     "--mean", "0.7833", "0.6712", "0.6026", "--std", "0.2139", "0.2472", "0.2571"]


@pytest.mark.parametrize("engine", ["fused", "compat"])
def test_backbone_train_runs_an_epoch_of_real_data(tree, tmp_path, engine, capsys):
    bt = _tool("backbone_train")
    # train split: 17 cases, -b 6: batches of 6, 6, 5 -- the partial last batch is trained
    args = bt.get_parser().parse_args(DATA(tree) + ["-a", "resnet18", "--arch-version", "v32", "-b", "6", "--img-sz", "64",
                                                    "64", "--epochs", "1", "--print-freq", "1", "--engine", engine,
                                                    "--log-path", str(tmp_path), "--temperature", "0.1"])
    args.world_size = 1
    hist = bt.main(0, args)
    out = capsys.readouterr().out
    assert len(hist) == 1 and math.isfinite(hist[0]), hist
    assert "[0][2/3]" in out and "image store: 34 images" in out, out
    ck = torch.load(os.path.join(str(tmp_path), "checkpoint.pth.tar"), map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and any(k.startswith("derm_backbone.encoder.") for k in ck["state_dict"])


def test_backbone_eval_validates_on_the_test_split_with_real_labels(tree, tmp_path):
    from sm3hip.metrics import auc_avg
    from src.utils.data.datasets import read_split
    be = _tool("backbone_eval")
    hist = be.main(DATA(tree) + ["-a", "resnet18", "-b", "6", "--img-sz", "64", "64", "--epochs", "1", "--finetune", "fc",
                                 "--log-path", str(tmp_path)])
    tr, va = hist[0]
    assert math.isfinite(tr["loss"]) and math.isfinite(va["loss"])
    saved = torch.load(os.path.join(str(tmp_path), "val_predictions.pt"), map_location="cpu", weights_only=False)
    labels = read_split(str(tree), "test")[2]
    assert torch.equal(saved["targets"], labels)             # the test split's real labels, in order
    assert all(p.shape[0] == len(labels) for p in saved["preds"])
    _, avg = auc_avg([p.to(DEV) for p in saved["preds"]], labels.to(DEV))    # where the tool computed it
    assert va["AUC_AVG"] == saved["AUC_AVG"] and abs(float(avg) - va["AUC_AVG"]) <= 1e-12, (float(avg), va["AUC_AVG"])


def test_mlc_train_then_mlc_eval_on_real_data(tree, tmp_path):
    from src.utils.data.datasets import read_split
    mt, me = _tool("mlc_train"), _tool("mlc_eval")
    n_train = len(read_split(str(tree), "train")[2])
    args = mt.get_parser().parse_args(DATA(tree) + ["-b", "6", "--img-sz", "64", "64", "--epochs", "1", "--temperature", "1",
                                                    "--mlc-proj-dim", "128", "--sa-dim-ff", "64", "--save-freq", "1",
                                                    "--log-path", str(tmp_path / "train")])
    args.world_size = 1
    args.probe = {}
    hist = mt.main(0, args)
    assert len(hist) == 1 and math.isfinite(hist[0])
    for a in args.probe["assignments"]:
        assert bool((a[:n_train] >= 0).all()), a               # every train index has a cluster
    hist = me.main(DATA(tree) + ["-b", "6", "--train-sz", "64", "--test-sz", "48", "--epochs", "1", "--mlc-proj-dim", "128",
                                 "--sa-dim-ff", "64", "--log-path", str(tmp_path / "eval"),
                                 "--pretrain-path", str(tmp_path / "train" / "ckp_0.pth")])
    tr, va = hist[0]
    assert math.isfinite(tr["loss"]) and math.isfinite(va["loss"]) and 0.0 <= va["AUC_AVG"] <= 1.0
    assert os.path.isfile(tmp_path / "eval" / "best_finetune.pth")
