"""GPU: test-time augmentation of the predictions (csrc/tta.hip, sm3hip/tta.py, the --tta flags of backbone_eval).

  * sm3_tta_dihedral == the torch expressions of the elements, bit for bit, around and past a tile edge, square and not;
  * store_views on a hand-built arena: view (c, g) == the torch expression of g on apply_ragged's output for crop c's box;
  * sm3_tta_reduce against the fp64 / integer restatement of tests/tta_inputs.py, edge rows, view permutations;
  * predict end to end on the ResNet-18 Baseline and the ResNet-50 inference.py Model: the views' logits == the model's own forward
    on the torch-made views, any chunk the same bits, the refusals;
  * predict_split over a hand-built store: five crops x flips, any batch size the same bits;
  * one run of backbone_eval.main with and without --tta d4 on synthetic data; each of the two tools on a derm7pt-shaped tree:
    val_predictions_tta.pt, read back through report.load_predictions and compared by eval_report --against --significance."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
DEV = "cuda:0"
MEAN, STD = [0.7833, 0.6712, 0.6026], [0.2139, 0.2472, 0.2571]


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TI = _load("sm3_tta_inputs_gpu", os.path.join(ROOT, "tests", "tta_inputs.py"))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- 1. the view expander ---------------------------------------------------------------------------------------------------
SQUARE = [(1, 1, 1), (2, 5, 5), (3, 31, 31), (2, 32, 32), (1, 33, 33), (1, 70, 70)]
OBLONG = [(2, 17, 9), (1, 9, 64)]


@pytest.mark.parametrize("B,H,W,group", [s + ("d4",) for s in SQUARE] + [s + ("flips",) for s in SQUARE + OBLONG] +
                         [SQUARE[2] + ("hflip",), OBLONG[0] + ("none",)])
def test_dihedral_equals_the_torch_expressions(B, H, W, group):
    from sm3hip import tta
    x = TI.distinct_images(B, H, W, seed=H * 100 + W)
    out = tta.dihedral(x.to(DEV), group)
    torch.cuda.synchronize()
    els = TI.GROUPS[group]
    assert out.shape == (B, len(els), 3, H, W) and out.dtype == torch.float32
    for gi, g in enumerate(els):
        assert torch.equal(_bits(out[:, gi]), _bits(TI.torch_view(x, g))), (g, H, W)


def test_dihedral_copies_bits_and_refuses_a_transpose_of_an_oblong_image():
    from sm3hip import _lib, ops, tta
    x = TI.distinct_images(1, 33, 33)
    x.view(-1)[:6] = torch.tensor([float("nan"), float("inf"), -float("inf"), -0.0, 1e-45, -1e-45])
    x.view(torch.int32).view(-1)[6] = 0x7FC12345  # a NaN with a payload
    out = tta.dihedral(x.to(DEV), "d4")
    for g in range(8):
        assert torch.equal(_bits(out[:, g]), _bits(TI.torch_view(x, g)))
    xo = torch.zeros(2, 3, 17, 9, device=DEV)
    out = torch.full((2, 8, 3, 17, 9), 7.0, device=DEV)
    with pytest.raises(ValueError, match="square"):
        tta.dihedral(xo, "d4")
    with pytest.raises(ValueError, match="square"):
        ops.tta_dihedral(xo, list(range(8)), out)
    import ctypes as C
    rc = _lib.load().sm3_tta_dihedral(ops._ptr(xo), 2, 17, 9, (C.c_int * 8)(*range(8)), 8, ops._ptr(out), ops._stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool((out == 7.0).all())  # nothing launched


# ---- 2. the views of an image store -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    a, offset, hs, ws = TI.arena()
    return a.to(DEV), offset, hs, ws


INDEX = [0, 1, 2, 3, 4, 2]


def _resampled(arena, size, box_of):
    """apply_ragged's output for the box box_of(h, w) of every image of INDEX, with whole_image_params' other fields."""
    from sm3hip.augment import SimCLRAugment, whole_image_params
    a, offset, hs, ws = arena
    idx = torch.tensor(INDEX)
    p = whole_image_params(hs[idx], ws[idx])
    p.box = torch.tensor([box_of(int(hs[i]), int(ws[i])) for i in INDEX], dtype=torch.int32)
    return SimCLRAugment(size, MEAN, STD).apply_ragged(a, offset, hs, ws, torch.tensor(INDEX, dtype=torch.int32), p)


@pytest.mark.parametrize("size,group", [((17, 17), "d4"), ((32, 32), "d4"), ((9, 17), "flips")])
def test_store_views_on_a_hand_built_arena(arena, size, group):
    from sm3hip import tta
    a, offset, hs, ws = arena
    els = TI.GROUPS[group]
    for crops in (1, 5):
        for s in (0.8, 1.0):
            out = tta.store_views(a, offset, hs, ws, INDEX, size, MEAN, STD, group, crops, s)
            assert out.shape == (len(INDEX), crops * len(els), 3) + size
            for c in range(crops):
                R = _resampled(arena, size, (lambda h, w: (0, 0, h, w)) if crops == 1 else (lambda h, w: TI.boxes(h, w, s)[c]))
                for gi, g in enumerate(els):
                    assert torch.equal(_bits(out[:, c * len(els) + gi]), _bits(TI.torch_view(R.cpu(), g))), (crops, s, c, g)


def test_store_views_without_views_is_the_validation_batch(arena):
    from sm3hip import tta
    from sm3hip.augment import SimCLRAugment, whole_image_params
    a, offset, hs, ws = arena
    idx = torch.tensor(INDEX)
    for size in ((17, 17), (9, 17)):
        want = SimCLRAugment(size, MEAN, STD).apply_ragged(a, offset, hs, ws, idx.int(), whole_image_params(hs[idx], ws[idx]))
        got = tta.store_views(a, offset, hs, ws, INDEX, size, MEAN, STD, "none", 1)
        assert got.shape == (len(INDEX), 1, 3) + size and torch.equal(_bits(got[:, 0]), _bits(want))


# ---- 3. the reduction ---------------------------------------------------------------------------------------------------------
def _reduce(z):
    from sm3hip import tta
    out = tta.reduce(torch.from_numpy(z).to(DEV))
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy() for k in ("q", "sum_q", "min_q", "max_q", "view_class", "agg_class", "disagree")}
    got["preds"] = torch.cat(out["preds"], dim=1).cpu().numpy()
    assert [p.shape[1] for p in out["preds"]] == TI.NUM_CLASSES
    return got


def _check_reduce(z):
    B, V, _ = z.shape
    got = _reduce(z)
    dq = np.abs(got["q"] - TI.q_of(z)).max()
    print(f"reduce B={B} V={V}: max |q - q_ref| = {dq}, min preds = {got['preds'].min():.4f}")
    assert dq <= 1
    ints = TI.reduce_ints(got["q"], z)
    for k, want in ints.items():
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want), k
    want = TI.preds_of(got["sum_q"], V)
    assert got["preds"].dtype == np.float32 and np.isfinite(got["preds"]).all()
    assert (np.abs(got["preds"].astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    if V == 1:
        assert np.array_equal(got["agg_class"], ints["view_class"][:, 0]) and (got["disagree"] == 0).all()
    perm = np.random.default_rng(B * 100 + V).permutation(V)
    again = _reduce(np.ascontiguousarray(z[:, perm]))
    for k in ("sum_q", "min_q", "max_q", "agg_class", "disagree"):
        assert np.array_equal(again[k], got[k]), k
    assert np.array_equal(again["preds"].view(np.uint32), got["preds"].view(np.uint32))
    assert np.array_equal(again["q"], got["q"][:, perm]) and np.array_equal(again["view_class"], got["view_class"][:, perm])
    return got


@pytest.mark.parametrize("V", [1, 2, 8, 40])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_reduce_against_the_integer_restatement(B, V):
    _check_reduce(TI.random_logits(B, V, seed=B * 1000 + V))
    got = _check_reduce(TI.edge_logits(V, seed=V))
    assert (got["view_class"][0] == 0).all() and (got["agg_class"][0] == 0).all() and (got["disagree"][0] == 0).all()
    assert got["sum_q"][1, 0] == V * TI.ONE and got["sum_q"][1, 1] == 0 and got["agg_class"][1, 0] == 0
    assert got["preds"][1, 1] == np.float32(np.log(1.0 / (V * 4294967296.0))) and got["preds"][1, 0] == 0.0
    assert (got["q"][2, :, 5:8] == np.int64(np.rint(4294967296.0 / 3))).all() and got["agg_class"][2, 1] == 0


def test_reduce_takes_the_eight_tensors_and_refuses_bad_logits():
    from sm3hip import tta
    z = torch.from_numpy(TI.random_logits(4, 8, 2)).to(DEV)
    a, b = tta.reduce(z), tta.reduce(list(z.split(TI.NUM_CLASSES, dim=2)))
    assert all(torch.equal(a[k], b[k]) for k in ("q", "sum_q", "min_q", "max_q", "view_class", "agg_class", "disagree"))
    assert all(torch.equal(p, q) for p, q in zip(a["preds"], b["preds"]))
    z[2, 3, 4] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        tta.reduce(z)
    with pytest.raises(ValueError, match="V <= 64"):
        tta.reduce(torch.zeros(1, 65, 24, device=DEV))


# ---- 4. predict ---------------------------------------------------------------------------------------------------------------
def _baseline18():
    from src.models.baseline import Baseline
    torch.manual_seed(21)
    m = Baseline("resnet18", None)
    for b in (m.derm_backbone, m.clinic_backbone):
        b.sm3_dtype = torch.float32
    return m.to(DEV).eval(), lambda d, c: m([d, c]), 3


def _mlc50():
    import inference
    from src.models.projector import build_mlc_projectors
    torch.manual_seed(22)
    ext = inference.Extractor("resnet50")
    m = inference.Model(ext, build_mlc_projectors("v4", 4096, 512, 8), 512, False, 1, 128, 0.1)
    for b in (ext.derm_backbone, ext.clinic_backbone):
        b.sm3_dtype = torch.float32
    return m.to(DEV).eval(), lambda d, c: m(d, c), 2


def _pairs(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, H, W, generator=g).to(DEV), torch.randn(n, 3, H, W, generator=g).to(DEV)


_RECORD_KEYS = ("q", "sum_q", "min_q", "max_q", "view_class", "agg_class", "disagree")


def _same_record(a, b):
    return all(torch.equal(a[k], b[k]) for k in _RECORD_KEYS) and \
        all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a["preds"] + a["logits"], b["preds"] + b["logits"]))


@pytest.mark.parametrize("make", [_baseline18, _mlc50])
def test_predict_end_to_end(make):
    from sm3hip import tta
    model, forward, n = make()
    derm, clinic = _pairs(n, 32, 32, seed=n)
    with torch.no_grad():
        own = [o.float() for o in forward(derm, clinic)]
        none = tta.predict(model, derm, clinic, "none")
        assert none["views"] == 1 and none["group"] == "none"
        for t in range(8):
            diff = float((none["logits"][t][:, 0] - own[t]).abs().max())
            print(f"label {t}: max |predict(none) - forward| = {diff:.3e}")
        for t in range(8):
            assert none["logits"][t].shape == (n, 1, TI.NUM_CLASSES[t]) and torch.equal(_bits(none["logits"][t][:, 0]), _bits(own[t]))
        assert all(torch.equal(none["agg_class"][:, t], own[t].argmax(dim=1)) for t in range(8))
        rec = tta.predict(model, derm, clinic, "d4")
        assert rec["views"] == 8 and rec["q"].shape == (n, 8, 24) and len(rec["preds"]) == 8
        for g in range(8):
            dv, cv = (TI.torch_view(x.cpu(), g).to(DEV) for x in (derm, clinic))
            for t, o in enumerate(forward(dv, cv)):
                assert torch.equal(_bits(rec["logits"][t][:, g]), _bits(o.float())), (g, t)
        one = tta.predict(model, derm, clinic, "d4", chunk=1)
    assert _same_record(rec, one)
    again = tta.reduce(rec["logits"])
    assert all(torch.equal(again[k], rec[k]) for k in _RECORD_KEYS)
    for t in range(8):  # softmax(preds) is the mean of the views' probabilities
        mean_p = torch.softmax(rec["logits"][t].double(), dim=2).mean(dim=1)
        assert float((torch.softmax(rec["preds"][t].double(), dim=1) - mean_p).abs().max()) < 1e-7


def test_predict_refuses_a_model_in_train_mode_and_an_oblong_image():
    from sm3hip import tta
    model, _, n = _baseline18()
    derm, clinic = _pairs(n, 32, 32, seed=4)
    with pytest.raises(ValueError, match="eval mode"):
        tta.predict(model.train(), derm, clinic, "d4")
    model.eval()
    with pytest.raises(ValueError, match="square"):
        tta.predict(model, derm[:, :, :, :16].contiguous(), clinic[:, :, :, :16].contiguous(), "d4")
    with pytest.raises(ValueError, match="chunk"):
        tta.predict(model, derm, clinic, "d4", chunk=0)
    with pytest.raises(ValueError, match="CUDA"):
        tta.predict(model, derm.cpu(), clinic.cpu(), "flips")
    rec = tta.predict(model, derm[:, :, :, :16].contiguous(), clinic[:, :, :, :16].contiguous(), "flips")  # 32 x 16: no transpose
    assert rec["views"] == 4 and rec["logits"][0].shape == (n, 4, 5)


def test_predict_split_over_a_hand_built_store(arena):
    """The image-store form: five crops x flips of 32 x 32 views; a view's logits == the model's forward on store_views' view;
    any batch size the same bits; crops = 1, group none == the validation batch through the model."""
    from types import SimpleNamespace
    from sm3hip import tta
    from sm3hip.imagestore import StoreSplit
    a, offset, hs, ws = arena
    store = SimpleNamespace(arena=a, offset=offset, img_h=hs, img_w=ws)
    derm_ids, clinic_ids = torch.tensor([0, 2, 4, 3, 1], dtype=torch.int32), torch.tensor([3, 3, 1, 0, 2], dtype=torch.int32)
    labels = torch.stack([torch.arange(5) % n for n in TI.NUM_CLASSES], dim=1).to(DEV)
    split = StoreSplit(derm_ids, clinic_ids, labels)
    model, forward, _ = _baseline18()
    rec = tta.predict_split(model, store, split, (32, 32), MEAN, STD, "flips", 5, 0.8, batch_size=2)
    assert rec["views"] == 20 and rec["crops"] == 5 and torch.equal(rec["targets"], labels) and rec["q"].shape == (5, 20, 24)
    dv, cv = (tta.store_views(a, offset, hs, ws, ids, (32, 32), MEAN, STD, "flips", 5, 0.8) for ids in (derm_ids, clinic_ids))
    with torch.no_grad():
        for v in (0, 3, 6, 19):
            for t, o in enumerate(forward(dv[:, v].contiguous(), cv[:, v].contiguous())):
                assert torch.equal(_bits(rec["logits"][t][:, v]), _bits(o.float())), (v, t)
    assert _same_record(rec, tta.predict_split(model, store, split, (32, 32), MEAN, STD, "flips", 5, 0.8, batch_size=64))
    none = tta.predict_split(model, store, split, (32, 32), MEAN, STD, "none", 1, 0.8, batch_size=3)
    from sm3hip.augment import SimCLRAugment, whole_image_params
    aug = SimCLRAugment((32, 32), MEAN, STD)
    val = [aug.apply_ragged(a, offset, hs, ws, ids, whole_image_params(hs[ids.long()], ws[ids.long()])) for ids in (derm_ids, clinic_ids)]
    with torch.no_grad():
        for t, o in enumerate(forward(*val)):
            assert torch.equal(_bits(none["logits"][t][:, 0]), _bits(o.float())), t
    with pytest.raises(ValueError, match="square"):
        tta.predict_split(model, store, split, (32, 16), MEAN, STD, "d4")


# ---- 5. the tools -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """A derm7pt-shaped directory (the fixture's metadata, small random PNG images) and the command line that reads it."""
    knn = _load("sm3_tta_knn_helpers", os.path.join(ROOT, "tests", "test_knn_gpu.py"))
    root = knn._write_tree(tmp_path_factory.mktemp("tta") / "7PC")
    return root, ["--data-name", "SevenPCBaseDataset", "--data-path", str(root), "-j", "4", "--mean"] + [str(m) for m in MEAN] + \
        ["--std"] + [str(s) for s in STD]


def _keep_records(tool, monkeypatch):
    """The records of the tool's TTA passes, as they are made."""
    records, tta_pass = [], tool.eval_cli.tta_pass
    monkeypatch.setattr(tool.eval_cli, "tta_pass", lambda *a, **k: records.append(tta_pass(*a, **k)) or records[-1])
    return records


def test_backbone_eval_on_a_derm7pt_tree(tree, tmp_path, capsys, monkeypatch):
    """Real data: val_predictions_tta.pt has val_predictions.pt's keys plus "tta", loads through report.load_predictions, and
    eval_report compares it with the plain file; val_predictions.pt itself is what the tool writes without the flag."""
    from sm3hip import report
    from src.utils.data.datasets import read_split
    root, data = tree
    labels = read_split(str(root), "test")[2]
    be = _load("sm3_tta_backbone_eval_tree", os.path.join(TOOLS, "backbone_eval.py"))
    records = _keep_records(be, monkeypatch)
    run = lambda extra, out: be.main(data + ["-a", "resnet18", "-b", "6", "--img-sz", "32", "32", "--epochs", "1", "--finetune",
                                             "fc", "--seed", "3", "--log-path", str(tmp_path / out)] + extra)
    run([], "plain")
    run(["--tta", "flips", "--tta-crops", "5", "--tta-crop-scale", "0.9"], "tta")
    out = capsys.readouterr().out
    assert out.count("val-tta AUC_AVG") == 1 and "tta flips x 5 crops = 20 views" in out
    plain = torch.load(tmp_path / "plain" / "val_predictions.pt", weights_only=False)
    same = torch.load(tmp_path / "tta" / "val_predictions.pt", weights_only=False)
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(plain["preds"], same["preds"]))  # the ordinary pass is untouched
    assert sorted(os.listdir(tmp_path / "tta")) == sorted(os.listdir(tmp_path / "plain") + ["val_predictions_tta.pt"])
    saved = torch.load(tmp_path / "tta" / "val_predictions_tta.pt", weights_only=False)
    assert len(records) == 1 and not torch.equal(records[0]["logits"][0][:, 0], records[0]["logits"][0][:, 1])  # views differ
    assert sorted(saved) == ["AUC_AVG", "epoch", "preds", "targets", "tta"] and torch.equal(saved["targets"], labels)
    t = saved["tta"]
    assert sorted(t) == sorted(["group", "crops", "crop_scale", "views", "sum_q", "min_q", "max_q", "disagree", "stability"])
    assert (t["group"], t["crops"], t["crop_scale"], t["views"]) == ("flips", 5, 0.9, 20)
    N = len(labels)
    assert t["sum_q"].shape == (N, 24) and t["disagree"].shape == (N, 8) and int(t["disagree"].max()) <= 20
    assert bool((t["min_q"] <= t["max_q"]).all()) and bool((t["sum_q"] <= 20 * t["max_q"]).all())
    assert all(torch.equal(t[k], records[0][k].cpu()) for k in ("sum_q", "min_q", "max_q", "disagree"))
    want = TI.preds_of(t["sum_q"].numpy(), 20)
    got = torch.cat(saved["preds"], dim=1).numpy()
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    preds, tg = report.load_predictions(str(tmp_path / "tta" / "val_predictions_tta.pt"))
    assert torch.equal(tg, labels) and all(torch.equal(p, q) for p, q in zip(preds, saved["preds"]))
    er = _load("sm3_tta_eval_report", os.path.join(TOOLS, "eval_report.py"))
    er.main([str(tmp_path / "tta" / "val_predictions_tta.pt"), "--against", str(tmp_path / "plain" / "val_predictions.pt"),
             "--significance", "--permutations", "200", "--out", str(tmp_path / "er")])
    assert "AUC difference" in capsys.readouterr().out
    with pytest.raises(SystemExit, match="real data"):
        be.main(["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "--tta", "flips", "--tta-crops", "5"])


def test_mlc_eval_on_a_derm7pt_tree(tree, tmp_path, capsys, monkeypatch):
    """The multi-label tool: the TTA pass runs inference.py's form of the evaluator, whose view 0 (d4's identity at one crop: the
    validation image) has the logits of the ordinary validation pass, bit for bit."""
    from src.utils.data.datasets import read_split
    root, data = tree
    labels = read_split(str(root), "test")[2]
    me = _load("sm3_tta_mlc_eval_tree", os.path.join(TOOLS, "mlc_eval.py"))
    records = _keep_records(me, monkeypatch)
    me.main(data + ["-b", "6", "--train-sz", "32", "--test-sz", "32", "--epochs", "1", "--mlc-proj-dim", "128", "--sa-dim-ff", "64",
                    "--tta", "d4", "--log-path", str(tmp_path)])
    assert "val-tta AUC_AVG" in capsys.readouterr().out and len(records) == 1
    saved = torch.load(tmp_path / "val_predictions_tta.pt", weights_only=False)
    plain = torch.load(tmp_path / "val_predictions.pt", weights_only=False)
    for t in range(8):
        assert torch.equal(_bits(records[0]["logits"][t][:, 0]), _bits(plain["preds"][t].float())), t
    assert saved["tta"]["views"] == 8 and torch.equal(saved["targets"], labels) and saved["tta"]["crops"] == 1
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(saved["preds"], records[0]["preds"]))


def test_backbone_eval_prints_the_tta_line_only_when_asked(tmp_path, capsys):
    be = _load("sm3_tta_backbone_eval", os.path.join(TOOLS, "backbone_eval.py"))
    base = ["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "-b", "4", "--img-sz", "32", "32", "--epochs", "1",
            "--steps-per-epoch", "1", "--val-steps", "1", "--finetune", "fc"]
    be.main(base + ["--log-path", str(tmp_path / "plain")])
    plain = capsys.readouterr().out
    assert "val-tta" not in plain and "epoch 0: val " in plain
    be.main(base + ["--log-path", str(tmp_path / "tta"), "--tta", "d4"])
    out = capsys.readouterr().out
    line = [l for l in out.splitlines() if l.startswith("epoch 0: val-tta AUC_AVG ")]
    assert len(line) == 1 and " | tta d4 x 1 crops = 8 views: flip_rate " in line[0] and "mean_range" in line[0]
    files = sorted(os.listdir(tmp_path / "plain"))
    assert files == sorted(os.listdir(tmp_path / "tta")) == ["best_linear.pth", "val_report.csv", "val_report.json"]
