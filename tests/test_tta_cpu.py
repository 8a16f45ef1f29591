"""CPU: test-time augmentation of the predictions (sm3hip/tta.py) -- the definitions, the refusals that need no device, the integer
restatement of the reduction (tests/tta_inputs.py), the stability values and the tools' flags."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TI = _load("sm3_tta_inputs_cpu", os.path.join(ROOT, "tests", "tta_inputs.py"))


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library or of a CUDA tensor fails the test."""
    from sm3hip import _lib

    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(torch.Tensor, "cuda", boom)


def test_the_eight_elements_are_distinct_and_equal_their_torch_expressions():
    R = torch.arange(25.0).view(5, 5)
    views = [TI.torch_view(R, g) for g in range(8)]
    for g in range(8):
        assert torch.equal(views[g], TI.index_view(R, g)), g
    assert len({tuple(v.reshape(-1).tolist()) for v in views}) == 8
    assert torch.equal(views[0], R) and torch.equal(views[1], R.flip(-1)) and torch.equal(views[2], R.flip(-2))
    assert torch.equal(views[3], R.flip(-1, -2)) and torch.equal(views[4], R.t())
    R = torch.arange(3 * 4 * 7.0).view(3, 4, 7)  # the mirrored elements of a non-square image
    for g in range(4):
        assert torch.equal(TI.torch_view(R, g), TI.index_view(R, g)), g


def test_groups_and_view_order():
    from sm3hip import tta
    assert list(tta.GROUPS) == ["none", "hflip", "flips", "d4"]
    assert tta.GROUPS == TI.GROUPS and all(tta.elements(n) == TI.GROUPS[n] for n in TI.GROUPS)
    assert [tta.n_views(n) for n in tta.GROUPS] == [1, 2, 4, 8] and tta.n_views("d4", 5) == 40 and tta.n_views("flips", 5) == 20
    # v = c * |G| + gi
    assert [(v // 4, tta.elements("flips")[v % 4]) for v in range(tta.n_views("flips", 5))] == \
        [(c, g) for c in range(5) for g in (0, 1, 2, 3)]
    with pytest.raises(ValueError, match="group"):
        tta.elements("rot90")
    with pytest.raises(ValueError, match="crops"):
        tta.n_views("d4", 3)


@pytest.mark.parametrize("s", [1.0, 0.8, 0.01])
def test_the_five_boxes_lie_inside_the_image(s):
    from sm3hip import tta
    sizes = [(1, 1), (2, 3), (37, 73), (301, 33)]
    box = tta.five_crop_boxes([h for h, _ in sizes], [w for _, w in sizes], s)
    assert box.shape == (5, 4, 4) and box.dtype == torch.int32
    for b, (h, w) in enumerate(sizes):
        assert [tuple(int(v) for v in box[c, b]) for c in range(5)] == TI.boxes(h, w, s)
        for c in range(5):
            i, j, ch, cw = (int(v) for v in box[c, b])
            assert ch >= 1 and cw >= 1 and i >= 0 and j >= 0 and i + ch <= h and j + cw <= w
        if s == 1.0:
            assert all(tuple(int(v) for v in box[c, b]) == (0, 0, h, w) for c in range(5))
    assert [tuple(int(v) for v in r) for r in tta.five_crop_boxes([37], [73], 0.8)[:, 0]] == \
        [(3, 7, 30, 58), (0, 0, 30, 58), (0, 15, 30, 58), (7, 0, 30, 58), (7, 15, 30, 58)]
    for bad in (0, -0.5, 1.01, float("nan"), True, "0.8"):
        with pytest.raises(ValueError, match="crop_scale"):
            tta.five_crop_boxes([4], [4], bad)


def _args(**kw):
    base = dict(tta="none", tta_crops=1, tta_crop_scale=0.8, img_sz=[224, 224])
    base.update(kw)
    return SimpleNamespace(**base)


def test_check_flags_refuses_without_a_device(no_device):
    from sm3hip import tta
    tta.check_flags(_args(), False)
    tta.check_flags(_args(tta="d4"), False)
    tta.check_flags(_args(tta="flips", img_sz=[224, 160]), False)
    tta.check_flags(_args(tta="d4", tta_crops=5, tta_crop_scale=1.0), True)
    tta.check_flags(_args(tta="d4", img_sz=[224, 160]), True, size=(96, 96))
    with pytest.raises(SystemExit, match="square"):
        tta.check_flags(_args(tta="d4", img_sz=[224, 160]), False)
    with pytest.raises(SystemExit, match="square"):
        tta.check_flags(_args(tta="d4"), True, size=(96, 64))
    with pytest.raises(SystemExit, match="real data"):
        tta.check_flags(_args(tta="flips", tta_crops=5), False)
    for bad in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(SystemExit, match="crop_scale"):
            tta.check_flags(_args(tta="hflip", tta_crop_scale=bad), True)


def test_reduce_and_dihedral_refuse_without_a_device(no_device):
    from sm3hip import tta
    z = torch.from_numpy(TI.random_logits(2, 4, 1))
    for bad in (float("nan"), float("inf"), float("-inf")):
        zb = z.clone()
        zb[1, 2, 7] = bad
        with pytest.raises(ValueError, match="finite"):
            tta.reduce(zb)
        with pytest.raises(ValueError, match="finite"):
            tta.reduce(list(zb.split(TI.NUM_CLASSES, dim=2)))
    with pytest.raises(ValueError, match="CUDA"):
        tta.reduce(z)  # the HIP path has no CPU fallback
    with pytest.raises(ValueError, match="24"):
        tta.reduce(z[:, :, :23])
    with pytest.raises(ValueError, match="V <= 64"):
        tta.reduce(torch.zeros(1, 65, 24))
    with pytest.raises(ValueError, match="8 tensors"):
        tta.reduce(list(z.split(TI.NUM_CLASSES, dim=2))[:7])
    with pytest.raises(ValueError, match="square"):
        tta.dihedral(torch.zeros(1, 3, 17, 9), "d4")
    with pytest.raises(ValueError, match="square"):
        tta.store_views(torch.zeros(8, dtype=torch.uint8), None, None, None, [0], (9, 17), [0.5] * 3, [0.2] * 3, "d4")
    with pytest.raises(ValueError, match="square"):
        tta.predict(object(), torch.zeros(1, 3, 17, 9), torch.zeros(1, 3, 17, 9), "d4")
    with pytest.raises(ValueError, match="CUDA"):
        tta.dihedral(torch.zeros(1, 3, 17, 9), "flips")


def test_library_refuses_on_the_host():
    """sm3_tta_dihedral / sm3_tta_reduce check their arguments before any launch: checkable without a GPU."""
    import ctypes as C
    from sm3hip import _lib
    lib = _lib.load()
    buf = C.c_void_p(64)  # never dereferenced: every call below is refused first
    els = lambda *g: (C.c_int * len(g))(*g)
    assert lib.sm3_tta_dihedral(None, 1, 4, 4, els(0), 1, buf, None) == -1
    assert lib.sm3_tta_dihedral(buf, 1, 4, 4, els(0), 1, None, None) == -1
    assert lib.sm3_tta_dihedral(buf, 1, 4, 4, None, 1, buf, None) == -1
    assert lib.sm3_tta_dihedral(buf, 1, 4, 4, els(0), 0, buf, None) == -1
    assert lib.sm3_tta_dihedral(buf, 1, 4, 4, els(*range(8), 0), 9, buf, None) == -1
    assert lib.sm3_tta_dihedral(buf, 1, 4, 4, els(8), 1, buf, None) == -1
    assert lib.sm3_tta_dihedral(buf, 1, 4, 4, els(-1), 1, buf, None) == -1
    assert lib.sm3_tta_dihedral(buf, 1, 17, 9, els(0, 4), 2, buf, None) == -1
    assert lib.sm3_tta_dihedral(buf, 0, 4, 4, els(0), 1, buf, None) == -1
    outs = [buf] * 8
    assert lib.sm3_tta_reduce(buf, 1, 0, *outs, None) == -1
    assert lib.sm3_tta_reduce(buf, 1, 65, *outs, None) == -1
    assert lib.sm3_tta_reduce(buf, 0, 8, *outs, None) == -1
    assert lib.sm3_tta_reduce(None, 1, 8, *outs, None) == -1
    assert lib.sm3_tta_reduce(buf, 1, 8, *outs[:7], None, None) == -1


@pytest.mark.parametrize("V", [1, 2, 8, 40])
def test_integer_restatement_is_invariant_under_a_permutation_of_the_views(V):
    z = np.concatenate([TI.random_logits(5, V, 3 + V), TI.edge_logits(V, 9)])
    z[3, :, :] = z[3, ::-1, :]  # views that really differ in order
    q = TI.q_of(z)
    assert q.min() >= 0 and q.max() <= TI.ONE
    for t in range(8):
        assert np.abs(q[..., TI.OFF[t]:TI.OFF[t + 1]].sum(axis=-1) - TI.ONE).max() <= 3  # a distribution, up to the roundings
    ref = TI.reduce_ints(q, z)
    perm = np.random.default_rng(V).permutation(V)
    got = TI.reduce_ints(TI.q_of(z[:, perm]), z[:, perm])
    assert np.array_equal(TI.q_of(z[:, perm]), q[:, perm])
    for k in ("sum_q", "min_q", "max_q", "agg_class", "disagree"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["view_class"], ref["view_class"][:, perm])
    # the edge rows: ties to the lowest index; the underflowing class keeps a finite prediction
    e = 5
    assert (ref["view_class"][e] == 0).all() and (ref["agg_class"][e] == 0).all() and (ref["disagree"][e] == 0).all()
    assert ref["sum_q"][e + 1, 1] == 0 and ref["sum_q"][e + 1, 0] == V * TI.ONE
    p = TI.preds_of(ref["sum_q"], V)
    assert np.isfinite(p).all() and p[e + 1, 1] == np.float32(np.log(1.0 / (V * 4294967296.0)))
    assert (ref["sum_q"][e + 2, 5:8] == V * np.int64(np.rint(4294967296.0 / 3))).all()
    if V == 40:
        assert abs(float(p.min()) + 25.87) < 0.01
    if V == 1:
        assert np.array_equal(ref["agg_class"], ref["view_class"][:, 0]) and (ref["disagree"] == 0).all()


def test_stability_on_a_hand_made_record():
    from sm3hip import tta
    N, V = 4, 8
    dis = torch.zeros(N, 8, dtype=torch.int64)
    dis[0, 0], dis[2, 0], dis[1, 7] = 3, 1, 8
    lo, hi = torch.zeros(N, 24, dtype=torch.int64), torch.zeros(N, 24, dtype=torch.int64)
    hi[:, 2] = torch.tensor([TI.ONE, TI.ONE // 2, 0, TI.ONE // 2])  # DIAG's scored class: column 0 + 2
    lo[:, 2] = torch.tensor([0, TI.ONE // 4, 0, TI.ONE // 2])
    hi[:, 23], lo[:, 23] = TI.ONE // 8, TI.ONE // 8 - 3                  # RS's scored class: column 22 + 1
    hi[:, 0] = TI.ONE                                                    # not a scored column: ignored
    s = tta.stability({"disagree": dis, "min_q": lo, "max_q": hi, "views": V})
    names = ["DIAG", "PN", "BWV", "VS", "PIG", "STR", "DaG", "RS"]
    assert list(s) == ["flip_rate", "mean_disagree", "mean_range"] and list(s["flip_rate"]) == names + ["AVG"]
    assert s["flip_rate"]["DIAG"] == 2 / 4 and s["flip_rate"]["RS"] == 1 / 4 and s["flip_rate"]["PN"] == 0.0
    assert s["flip_rate"]["AVG"] == (0.5 + 0.25) / 8
    assert s["mean_disagree"]["DIAG"] == 4 / 32 and s["mean_disagree"]["RS"] == 8 / 32 and s["mean_disagree"]["AVG"] == 0.375 / 8
    assert s["mean_range"]["DIAG"] == (1.0 + 0.25) / 4 and s["mean_range"]["RS"] == 12 / (4 * 2.0 ** 32)
    assert s["mean_range"]["AVG"] == (0.3125 + 12 / (4 * 2.0 ** 32)) / 8
    line = tta.stats_line({"disagree": dis, "min_q": lo, "max_q": hi, "views": V, "group": "d4"})
    assert "d4" in line and "8 views" in line and "flip_rate 0.0938" in line and "mean_range" in line


@pytest.mark.parametrize("name", ["backbone_eval", "mlc_eval"])
def test_the_tools_take_the_flags_and_default_to_none(name):
    parser = _load("sm3_tta_cli_" + name, os.path.join(TOOLS, name + ".py")).get_parser()
    base = ["--data-name", "synthetic", "--data-path", "-"]
    args = parser.parse_args(base)
    assert (args.tta, args.tta_crops, args.tta_crop_scale) == ("none", 1, 0.8)
    args = parser.parse_args(base + ["--tta", "d4", "--tta-crops", "5", "--tta-crop-scale", "0.9"])
    assert (args.tta, args.tta_crops, args.tta_crop_scale) == ("d4", 5, 0.9)
    for bad in (["--tta", "rot90"], ["--tta-crops", "3"]):
        with pytest.raises(SystemExit):
            parser.parse_args(base + bad)


def test_the_tools_on_frozen_features_and_the_explanation_tools_do_not_take_the_flags():
    for name in ("backbone_knn", "backbone_logreg", "backbone_cam"):
        parser = _load("sm3_tta_cli_" + name, os.path.join(TOOLS, name + ".py")).get_parser()
        with pytest.raises(SystemExit):
            parser.parse_args(["--data-name", "synthetic", "--data-path", "-", "--tta", "d4"])


def test_a_saved_file_with_the_tta_key_loads_as_any_predictions_file(tmp_path):
    from sm3hip import report, tta
    z = TI.random_logits(6, 8, 4)
    ints = TI.reduce_ints(TI.q_of(z), z)
    preds = list(torch.from_numpy(TI.preds_of(ints["sum_q"], 8)).split(TI.NUM_CLASSES, dim=1))
    targets = torch.stack([torch.arange(6) % n for n in TI.NUM_CLASSES], dim=1)
    rec = {k: torch.from_numpy(ints[k]) for k in ("sum_q", "min_q", "max_q", "disagree")}
    rec.update(group="d4", views=8, crops=1, crop_scale=0.8)
    path = tmp_path / "val_predictions_tta.pt"
    torch.save({"epoch": 1, "preds": preds, "targets": targets, "AUC_AVG": 0.5, "tta": tta.tool_record(rec)}, path)
    got, tg = report.load_predictions(str(path))
    assert all(torch.equal(a, b) for a, b in zip(got, preds)) and torch.equal(tg, targets)
    saved = torch.load(path, weights_only=False)["tta"]
    assert sorted(saved) == sorted(["group", "crops", "crop_scale", "views", "sum_q", "min_q", "max_q", "disagree", "stability"])
    # softmax(preds) is the mean probability of the views
    mean_p = ints["sum_q"] / (8 * 4294967296.0)
    for t in range(8):
        sm = torch.softmax(preds[t].double(), dim=1).numpy()
        assert np.abs(sm - mean_p[:, TI.OFF[t]:TI.OFF[t + 1]]).max() < 1e-6
