"""CPU: the derm7pt dataset mirror (src/utils/data/datasets.py) against what the reference's own SevenPCBaseDataset reads
from the same metadata (tests/golden/derm7pt_ref.npz, tests/golden/gen_derm7pt_golden.py), the tools' batch order against
torch's DistributedSampler, the ragged parameter draw, and the tools' up-front refusals."""
import os
import shutil
import types

import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
META = os.path.join(GOLDEN, "derm7pt_meta")
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")


def _args(path):
    return types.SimpleNamespace(data_path=path, workers=2)


def _copy_meta(tmp_path):
    d = tmp_path / "7PC"
    shutil.copytree(META, d)
    (d / "images").mkdir()
    return d


@pytest.mark.parametrize("mode", ["train", "val", "test"])
def test_labels_and_paths_equal_the_reference(mode):
    from src.utils.data.datasets import SevenPCBaseDataset
    ref = np.load(os.path.join(GOLDEN, "derm7pt_ref.npz"))
    ds = SevenPCBaseDataset(_args(META), None, mode)
    assert ds.labels.dtype == torch.int64 and ds.labels.shape == (len(ref[f"{mode}_labels"]), 8)
    assert np.array_equal(ds.labels.numpy(), ref[f"{mode}_labels"])
    images = os.path.join(META, "images")
    assert [os.path.relpath(p, images) for p in ds.derm_data] == list(ref[f"{mode}_derm"])
    assert [os.path.relpath(p, images) for p in ds.clinic_data] == list(ref[f"{mode}_clinic"])
    assert len(ds) == len(ref[f"{mode}_labels"])


def test_every_label_class_is_used_by_the_fixture():
    from src.utils.data.datasets import NUM_CLASSES
    ref = np.load(os.path.join(GOLDEN, "derm7pt_ref.npz"))
    labels = np.concatenate([ref[f"{m}_labels"] for m in ("train", "val", "test")])
    for c, n in enumerate(NUM_CLASSES):
        assert sorted(set(labels[:, c].tolist())) == list(range(n)), c


def test_unknown_label_raises_the_reference_message(tmp_path):
    from src.utils.data.datasets import SevenPCBaseDataset
    d = _copy_meta(tmp_path)
    meta = pd.read_csv(d / "meta.csv")
    meta.loc[0, "pigment_network"] = "faint"
    meta.to_csv(d / "meta.csv", index=False)
    want = str(np.load(os.path.join(GOLDEN, "derm7pt_ref.npz"))["unknown_label_message"])
    with pytest.raises(ValueError) as e:
        SevenPCBaseDataset(_args(str(d)), None, "train")
    assert str(e.value) == want


def test_overlapping_index_lists_fail_and_incomplete_ones_warn(tmp_path, capsys):
    from src.utils.data.datasets import SevenPCBaseDataset
    d = _copy_meta(tmp_path)
    train = pd.read_csv(d / "train_indexes.csv")["indexes"].tolist()
    test = pd.read_csv(d / "test_indexes.csv")["indexes"].tolist()
    pd.DataFrame({"indexes": test + train[:1]}).to_csv(d / "test_indexes.csv", index=False)
    with pytest.raises(ValueError, match="duplicate indexes"):
        SevenPCBaseDataset(_args(str(d)), None, "test")
    pd.DataFrame({"indexes": test[:-1]}).to_csv(d / "test_indexes.csv", index=False)
    ds = SevenPCBaseDataset(_args(str(d)), None, "test")
    assert len(ds) == len(test) - 1 and "Warning!" in capsys.readouterr().out


@pytest.mark.parametrize("n", [17, 30, 31])
def test_sampler_order_equals_torch_distributed_sampler(n):
    from src.utils.data.sampler import eval_batches, train_batches

    class DS:
        def __len__(self):
            return n

    for world in (1, 2):
        for rank in range(world):
            for epoch in range(3):
                s = torch.utils.data.DistributedSampler(DS(), num_replicas=world, rank=rank, shuffle=True, seed=0,
                                                        drop_last=False)
                s.set_epoch(epoch)
                want = list(s)
                got = train_batches(n, world, rank, epoch, 8)
                assert [len(b) for b in got[:-1]] == [8] * (len(got) - 1) and 0 < len(got[-1]) <= 8
                assert torch.cat(got).tolist() == want, (world, rank, epoch)
    ev = eval_batches(n, 8)
    assert torch.cat(ev).tolist() == list(range(n)) and [len(b) for b in ev[:-1]] == [8] * (len(ev) - 1)


def test_ragged_draw_keeps_the_fixed_size_stream_and_boxes_fit_each_image():
    from sm3hip.augment import CHAINS, SimCLRAugment, chain
    aug = SimCLRAugment(64, [0.5] * 3, [0.25] * 3)
    p = aug.sample(7, 90, 130, torch.Generator().manual_seed(4))
    q = aug.sample_ragged([90] * 7, [130] * 7, torch.Generator().manual_seed(4))
    for k in ("box", "flip", "ops", "factors", "gray", "sigma"):
        assert torch.equal(getattr(p, k), getattr(q, k)), k
    hs, ws = [300, 462, 560, 51, 700], [420, 718, 780, 900, 60]
    for tool in CHAINS:
        a = chain(tool, (32, 32), [0.5] * 3, [0.25] * 3)
        r = a.sample_ragged(hs, ws, torch.Generator().manual_seed(1))
        b = r.box
        assert bool((b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 2] > 0).all() and (b[:, 3] > 0).all())
        assert bool((b[:, 0] + b[:, 2] <= torch.tensor(hs)).all() and (b[:, 1] + b[:, 3] <= torch.tensor(ws)).all())
        if tool != "backbone_train":
            assert not bool(r.gray.any()) and not bool(r.sigma.any())
        if tool in ("backbone_eval", "mlc_eval"):
            assert not bool(r.ops.any())


def test_decode_applies_exif_orientation_and_refuses_tiny_images(tmp_path):
    from src.utils.data.datasets import load_rgb
    g = np.random.default_rng(0)
    a = g.integers(0, 256, (80, 120, 3), dtype=np.uint8)
    ex = Image.Exif()
    ex[0x0112] = 6                                           # rotate 90 degrees clockwise to display
    Image.fromarray(a).save(tmp_path / "r.png", exif=ex)
    got = load_rgb(str(tmp_path / "r.png"))
    assert np.array_equal(got, np.rot90(a, -1)[25:-25, 25:-25])
    Image.fromarray(a[:50]).save(tmp_path / "small.png")
    with pytest.raises(ValueError, match="small.png"):
        load_rgb(str(tmp_path / "small.png"))


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location("sm3_derm_" + name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tools_refuse_bad_data_before_any_kernel(tmp_path, monkeypatch):
    import torch.cuda
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("reached the device"))
    d = _copy_meta(tmp_path)
    no_meta, no_images = tmp_path / "a", tmp_path / "b"
    shutil.copytree(d, no_meta)
    os.remove(no_meta / "meta.csv")
    shutil.copytree(META, no_images)
    cases = [(["--data-name", "ISIC2018", "--data-path", str(d)], "not available"),
             (["--data-name", "SevenPCBaseDataset", "--data-path", str(no_meta)], "meta.csv"),
             (["--data-name", "SevenPCBaseDataset", "--data-path", str(no_images)], "images/")]
    for argv, msg in cases:
        for name in ("backbone_train", "mlc_train"):
            mod = _tool(name)
            args = mod.get_parser().parse_args(argv + ["--log-path", str(tmp_path / "logs")])
            args.world_size = 1
            with pytest.raises(SystemExit, match=msg):
                mod.main(0, args)
        for name, extra in (("backbone_eval", ["-a", "resnet18"]), ("mlc_eval", [])):
            with pytest.raises(SystemExit, match=msg):
                _tool(name).main(argv + extra + ["--log-path", str(tmp_path / "logs")])


def test_workers_leaves_the_ignored_line_only_with_a_real_dataset(tmp_path):
    from src.utils.misc import describe_ignored, ignored_line, require_data
    d = _copy_meta(tmp_path)
    parser = _tool("backbone_train").get_parser()
    syn = parser.parse_args(["--data-name", "synthetic", "--data-path", "-", "-j", "4", "--wandb"])
    real = parser.parse_args(["--data-name", "SevenPCBaseDataset", "--data-path", str(d), "-j", "4", "--wandb"])
    assert not require_data(syn, "t") and require_data(real, "t")
    assert describe_ignored(syn, parser) == describe_ignored(real, parser) == ["--workers", "--wandb"]
    assert ignored_line(syn, parser, False) == ["--workers", "--wandb"] and ignored_line(real, parser, True) == ["--wandb"]
