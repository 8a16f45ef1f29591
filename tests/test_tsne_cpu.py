"""CPU: exact t-SNE maps (sm3hip/tsne.py, csrc/tsne.hip, tools/backbone_map.py) -- what can be said without a device.

  * the quality condition on the numpy restatement (tests/tsne_ref.py): on blobs(300, 16, 6, 0), for every seed 0 .. 4,
    KL <= max_sk + (max_sk - min_sk) and trustworthiness >= min_sk - (max_sk - min_sk), where min_sk / max_sk are over the 20
    scikit-learn runs recorded in tests/golden/tsne_sklearn_ref.json.  The margin is the reference's own seed-to-seed spread:
    t-SNE trajectories are chaotic, no two implementations agree pointwise.  Both the fp64 pair arithmetic and the emulation of
    the kernel's fp32 pair arithmetic must meet it;
  * every row of the restatement's conditional P has perplexity within 1e-9 of the target; degenerate rows are uniform;
  * the fixed order against an exact sum; the host refusals with no device; header, binding and library carry the entry points,
    which refuse bad arguments before any launch;
  * the first maps ("random" is the restatement's, "pca" is signed and scaled as documented), preservation and partner ranks on
    hand-made maps; render writes a PNG of the asked size with the asked colours at the pixels pixel_coords names;
  * the tool's flags parse and its refusals fire before the device is touched."""
import ctypes as C
import importlib.util
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tsne_ref as R  # noqa: E402

SEEDS = (0, 1, 2, 3, 4)
ENTRY_POINTS = {"sm3_tsne_max_points": 0, "sm3_tsne_sqdist": 5, "sm3_tsne_affinities": 6, "sm3_tsne_symmetrise": 4,
                "sm3_tsne_forces": 5, "sm3_tsne_update": 10, "sm3_tsne_kl": 7}


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def quality_bounds():
    """(KL upper bound, trustworthiness lower bound, the recorded JSON) from the scikit-learn runs."""
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "tsne_sklearn_ref.json")))
    kl = [r["kl"] for r in ref["runs"]]
    tw = [r["trustworthiness"] for r in ref["runs"]]
    assert len(ref["runs"]) == 20 and ref["settings"]["method"] == "exact" and ref["n_neighbors"] == 10
    return max(kl) + (max(kl) - min(kl)), min(tw) - (max(tw) - min(tw)), ref


def golden_input():
    ref = quality_bounds()[2]
    x, labels = R.blobs(**ref["input"])
    assert float(x.astype(np.float64).sum()) == ref["input_checksum"]  # the input the scikit-learn runs saw
    return x, labels


# ---- the quality condition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arithmetic", ["fp64", "fp32"])
def test_restatement_meets_the_quality_condition(arithmetic):
    kl_max, tw_min, _ = quality_bounds()
    x, _ = golden_input()
    for seed in SEEDS:
        rep = R.tsne(x, seed=seed, arithmetic=arithmetic)
        tw = R.trustworthiness(x, rep["map"], 10)
        print(f"{arithmetic} seed {seed}: KL {rep['kl']:.5f} (<= {kl_max:.5f}), trustworthiness {tw:.5f} (>= {tw_min:.5f})")
        assert rep["iters_run"] == 1000 and len(rep["history"]) == 20
        assert rep["kl"] <= kl_max and tw >= tw_min, (seed, rep["kl"], tw)


def test_trustworthiness_of_hand_made_maps():
    x, _ = golden_input()
    assert R.trustworthiness(x, x, 10) == 1.0                                   # the map that keeps every neighbour
    y = np.random.RandomState(1).randn(300, 2)
    assert 0.4 < R.trustworthiness(x, y, 10) < 0.7                              # a map that knows nothing: about one half


# ---- the restatement's own properties -----------------------------------------------------------------------------------
def test_fixed_sum_is_the_documented_order():
    rs = np.random.RandomState(0)
    for n in (1, 3, 255, 256, 257, 600, 1000):
        t = rs.randn(n) * 10.0 ** rs.randint(-3, 4, n)
        part = [0.0] * 256
        for j in range(n):
            part[j % 256] += t[j]
        h = 128
        while h:
            for k in range(h):
                part[k] += part[k + h]
            h >>= 1
        assert R.fixed_sum(t) == part[0]
        assert abs(R.fixed_sum(t) - math.fsum(t)) <= n * 2.0 ** -52 * math.fsum(np.abs(t))
    assert np.array_equal(R.fixed_sum(np.arange(12.0).reshape(3, 4)), [6.0, 22.0, 38.0])


@pytest.mark.parametrize("perplexity", [2.0, 30.0, 299 / 3])
def test_conditional_rows_reach_the_perplexity(perplexity):
    x, _ = golden_input()
    c, beta = R.conditional(R.sqdist(x), perplexity)
    assert np.isfinite(c).all() and np.isfinite(beta).all() and (beta > 0).all() and not c.diagonal().any()
    assert np.abs(c.sum(axis=1) - 1.0).max() < 1e-12
    assert np.abs(R.row_perplexity(c) - perplexity).max() <= 1e-9
    P = R.symmetrise(c.astype(np.float32))
    assert np.array_equal(P, P.T) and abs(float(P.astype(np.float64).sum()) - 1.0) < 1e-6


def test_conditional_of_degenerate_rows():
    c, beta = R.conditional(np.zeros((7, 7)), 2.0)                               # all points equal: uniform, never NaN
    assert np.array_equal(c, (1.0 - np.eye(7)) / 6.0) and np.array_equal(beta, np.full(7, 2.0 ** 100))
    x = np.random.RandomState(0).randn(40, 4)
    x[1] = x[0]                                                                 # an exact duplicate pair: its least distance is 0
    c, _ = R.conditional(R.sqdist(x), 5.0)
    assert np.isfinite(c).all() and np.abs(R.row_perplexity(c) - 5.0).max() <= 1e-9


def test_update_follows_the_gradient_descent_rule():
    rs = np.random.RandomState(0)
    N = 9
    F = np.concatenate([rs.rand(N, 1) + 1.0, rs.randn(N, 4)], axis=1)
    y, u, g = rs.randn(N, 2).astype(np.float32), rs.randn(N, 2).astype(np.float32), (rs.rand(N, 2) * 2).astype(np.float32)
    g[0, 0] = 0.011                                                             # x 0.8 falls under the floor
    y1, u1, g1, grad, gn2, Z = R.update(F, 12.0, 0.5, 200.0, y, u, g)
    want = 4.0 * (12.0 * F[:, 1:3] - F[:, 3:5] / F[:, 0].sum())
    assert np.allclose(grad, want, rtol=1e-14, atol=0) and abs(Z - F[:, 0].sum()) < 1e-12
    inc = u.astype(np.float64) * grad < 0
    gains = np.maximum(np.where(inc, g.astype(np.float64) + 0.2, g.astype(np.float64) * 0.8), 0.01)
    assert np.array_equal(g1, gains.astype(np.float32)) and (g1 >= np.float32(0.01)).all()
    assert np.array_equal(u1, (0.5 * u.astype(np.float64) - 200.0 * gains * grad).astype(np.float32))
    assert np.allclose(y1, y + u1, rtol=1e-6) and abs(gn2 - ((gains * grad) ** 2).sum()) < 1e-9 * gn2


# ---- the library --------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_carry_the_entry_points():
    from sm3hip import _lib, ops, tsne
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sm3_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        declared = 0 if m.group(1).strip() == "void" else len(m.group(1).split(","))
        assert declared == len(_lib.SIGNATURES[name]) == nargs, name
        assert hasattr(lib, name)
    assert lib.sm3_abi_version() == 9
    assert lib.sm3_tsne_max_points() == tsne.MAX_POINTS == ops.TSNE_MAX_POINTS == R.MAX_POINTS == 16384


def test_entry_points_reject_bad_arguments_before_any_launch():
    from sm3hip import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)  # host memory: never dereferenced by a kernel, every call below returns before a launch
    q = C.c_void_p(p.value + 256)
    odd, odd2 = C.c_void_p(p.value + 4), C.c_void_p(p.value + 2)  # not 8-byte / not 4-byte aligned
    calls = {
        "sqdist": (lambda x=p, N=5, D=3, d2=q: lib.sm3_tsne_sqdist(x, N, D, d2, None), ("x", "d2")),
        "affinities": (lambda d2=p, N=5, perplexity=1.2, cond=q, beta=p: lib.sm3_tsne_affinities(d2, N, perplexity, cond, beta, None),
                       ("d2", "cond", "beta")),
        "symmetrise": (lambda cond=p, N=5, P=q: lib.sm3_tsne_symmetrise(cond, N, P, None), ("cond", "P")),
        "forces": (lambda P=p, y=q, N=5, F=p: lib.sm3_tsne_forces(P, y, N, F, None), ("P", "y", "F")),
        "update": (lambda F=p, N=5, e=12.0, m=0.5, lr=200.0, y=q, update=q, gains=q, out=p:
                   lib.sm3_tsne_update(F, N, e, m, lr, y, update, gains, out, None), ("F", "y", "update", "gains", "out")),
        "kl": (lambda P=p, y=q, F=p, N=5, rows=p, out=p: lib.sm3_tsne_kl(P, y, F, N, rows, out, None),
               ("P", "y", "F", "rows", "out")),
    }
    for name, (call, pointers) in calls.items():
        for arg in pointers:
            assert call(**{arg: None}) == -1, (name, arg)
        for N in (3, 0, -1, 16385):
            assert call(N=N) == -1, (name, N)
    sq, aff, sym, frc, upd, kl = (calls[k][0] for k in ("sqdist", "affinities", "symmetrise", "forces", "update", "kl"))
    assert sq(D=0) == -1 and sq(D=4097) == -1 and sq(x=odd2) == -2 and sq(d2=odd2) == -2
    assert aff(perplexity=0.5) == -1 and aff(perplexity=4.5) == -1 and aff(perplexity=float("nan")) == -1 and aff(beta=odd) == -2
    assert sym(P=p) == -1 and sym(P=odd2) == -2
    assert frc(y=odd) == -2 and frc(F=odd) == -2
    assert upd(e=float("inf")) == -1 and upd(m=float("nan")) == -1 and upd(lr=float("inf")) == -1 and upd(out=odd) == -2
    assert kl(rows=odd) == -2 and kl(y=odd) == -2


def test_host_refusals_with_no_device():
    from sm3hip import tsne
    x = torch.randn(40, 8)
    bad = x.clone()
    bad[3, 2] = float("nan")
    inf = x.clone()
    inf[0, 0] = float("inf")
    for fn in (tsne.tsne, tsne.affinities):
        for t in (bad, inf):
            with pytest.raises(ValueError, match="not finite"):
                fn(t)
        for t in (x.double(), x[0], x.numpy()):
            with pytest.raises(ValueError, match="2-D float32"):
                fn(t)
        with pytest.raises(ValueError, match=f"MAX_POINTS = {tsne.MAX_POINTS}"):
            fn(torch.zeros(3, 8), 1.0)
        with pytest.raises(ValueError, match=f"MAX_POINTS = {tsne.MAX_POINTS}"):
            fn(torch.zeros(tsne.MAX_POINTS + 1, 1), 30.0)
        with pytest.raises(ValueError, match="features"):
            fn(torch.zeros(40, tsne.MAX_DIM + 1), 5.0)
        for perplexity in (0.99, 13.01, 30.0, float("nan"), "30", True):           # (N - 1) / 3 = 13
            with pytest.raises(ValueError, match="perplexity"):
                fn(x, perplexity)
        with pytest.raises(ValueError, match="GPU"):                               # everything else is fine: only the device is not
            fn(x, 13.0)
    for kw in ({"iters": 0}, {"iters": 10.0}, {"exaggeration": 0.5}, {"exaggeration": float("inf")}, {"exaggeration_iters": -1},
               {"learning_rate": 0}, {"learning_rate": "fast"}, {"init": "spectral"}, {"seed": -1}, {"seed": 1.5},
               {"check_every": 0}, {"min_grad_norm": -1.0}, {"patience": -1}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            tsne.check_settings(**{**dict(iters=1000, exaggeration=12.0, exaggeration_iters=250, learning_rate="auto",
                                          init="random", seed=0, check_every=50, min_grad_norm=1e-7, patience=300), **kw})
    with pytest.raises(ValueError, match="initial map"):
        tsne.initial_map(x, np.zeros((39, 2)), 0)
    with pytest.raises(ValueError, match="same cases"):
        tsne.cross_modal_map(x, x[:10])
    with pytest.raises(ValueError, match="2-D float32"):
        tsne.cross_modal_map(x, x.double())


# ---- first maps, neighbours, ranks --------------------------------------------------------------------------------------
def test_first_maps():
    from sm3hip import tsne
    x = torch.from_numpy(golden_input()[0])
    for seed in (0, 7):
        y = tsne.initial_map(x, "random", seed)
        assert y.dtype == torch.float32 and np.array_equal(y.numpy(), R.random_init(300, seed))
    given = np.arange(600.0).reshape(300, 2)
    assert np.array_equal(tsne.initial_map(x, given, 0).numpy(), given.astype(np.float32))
    y = tsne.pca_init(x).double().numpy()
    assert y.shape == (300, 2) and abs(y[:, 0].std() - 1e-4) < 1e-9 and y[:, 0].std() >= y[:, 1].std() > 0
    xc = x.double().numpy() - x.double().numpy().mean(axis=0)
    axes, *_ = np.linalg.lstsq(xc, y, rcond=None)                                  # y = xc @ axes: recover the axes; y is fp32
    assert abs(float(axes[:, 0] @ axes[:, 1])) < 1e-6 * float(axes[:, 0] @ axes[:, 0])
    for a in axes.T:
        assert a[np.abs(a).argmax()] > 0                                          # the largest-magnitude loading is positive
    top = np.linalg.eigvalsh(xc.T @ xc)[::-1][:2]
    assert np.allclose((xc @ (axes / np.linalg.norm(axes, axis=0))).var(axis=0) * 300, top, rtol=1e-5)
    assert np.array_equal(tsne.pca_init(-x).numpy(), -tsne.pca_init(x).numpy())   # the axes keep their sign, the points flip
    with pytest.raises(ValueError, match="two features"):
        tsne.pca_init(x[:, :1])


def test_preservation_and_partner_ranks_on_hand_made_maps():
    from sm3hip import tsne
    x = torch.from_numpy(golden_input()[0])
    assert tsne.preservation(x, x[:, :], 10) == 1.0
    line = torch.arange(8.0)[:, None] * torch.tensor([[1.0, 0.0]])
    assert tsne.preservation(line, line * 3.0, 2) == 1.0
    rev = line[[0, 7, 1, 6, 2, 5, 3, 4]]
    assert 0.0 <= tsne.preservation(line, rev, 2) < 1.0
    with pytest.raises(ValueError, match="preservation"):
        tsne.preservation(line, line, 8)
    derm = torch.tensor([[0.0, 0.0], [10.0, 0.0], [20.0, 0.0]])
    clinic = torch.tensor([[0.0, 1.0], [10.0, 25.0], [20.0, 1.0]])
    # case 1: from its derm point everything else is nearer than its partner; from its clinical point the partner is nearest
    assert tsne.partner_ranks(derm, clinic).tolist() == [[1, 1], [5, 1], [1, 1]]
    same = torch.zeros(2, 2)
    assert tsne.partner_ranks(same, same).tolist() == [[2, 1], [3, 2]]            # every distance tied: the lower index first


# ---- render -------------------------------------------------------------------------------------------------------------
def test_render_writes_the_asked_picture(tmp_path):
    from PIL import Image
    from sm3hip import tsne
    y = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 2.0], [1.0, 1.0], [1.0, 1.0]])
    colours = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [9, 9, 9], [250, 128, 1]])
    for size in (64, 257):
        path = tmp_path / f"m{size}.png"
        px = tsne.render(y, colours, str(path), size=size, pair_lines=[[0, 2]])
        assert np.array_equal(px, tsne.pixel_coords(y, size))
        im = Image.open(path)
        assert im.format == "PNG" and im.size == (size, size) and im.mode == "RGB"
        a = np.asarray(im)
        m, r = size // 32, tsne.point_radius(size)
        assert px[0, 0] == m and px[1, 0] == size - 1 - m and px[1, 1] == px[0, 1] and px[2, 1] < px[1, 1]
        for n in (0, 1, 2, 4):                                                     # point 4 covers point 3: index order
            cx, cy = px[n]
            assert (a[cy - r:cy + r + 1, cx - r:cx + r + 1] == colours[n]).all(), n
        assert not (a == 9).all(axis=2).any()
        assert (a[0, 0] == 255).all() and (a[size - 1, size - 1] == 255).all()
        grey = (a == np.array(tsne.LINE)).all(axis=2)
        assert grey.any()                                                          # the pair line is there, under the points
        tsne.render(y, colours, str(path), size=size)
        assert not (np.asarray(Image.open(path)) == np.array(tsne.LINE)).all(axis=2).any()
    one = tsne.render(np.zeros((3, 2)), colours[:3], str(tmp_path / "one.png"), size=64)   # no extent: the centre
    assert (one[:, 0] == one[0, 0]).all() and 30 <= one[0, 0] <= 33
    for bad in (dict(map=y[:, :1]), dict(colours=colours[:4]), dict(colours=colours * 2), dict(size=8), dict(pair_lines=[[0, 5]])):
        kw = {**dict(map=y, colours=colours, path=str(tmp_path / "bad.png"), size=64), **bad}
        with pytest.raises(ValueError, match="render"):
            tsne.render(**kw)
    assert tsne.class_colours([0, 1, 9]).tolist() == [list(tsne.PALETTE[0]), list(tsne.PALETTE[1]), list(tsne.PALETTE[1])]


# ---- the tool -----------------------------------------------------------------------------------------------------------
def _tool(name):
    return _load("sm3_tsne_cli_" + name, os.path.join(TOOLS, name + ".py"))


def test_backbone_map_parses_its_flags():
    p = _tool("backbone_map").get_parser()
    base = ["--data-name", "synthetic", "--data-path", "-"]
    d = p.parse_args(base)
    assert (d.perplexity, d.map_iters, d.map_init, d.map_seed) == (30.0, 1000, "random", 0)
    assert d.embeddings is None and d.colour_by == "modality" and d.pair_lines is False and d.arch_version == "v3"
    a = p.parse_args(base + ["--perplexity", "12.5", "--map-iters", "300", "--map-init", "pca", "--map-seed", "9", "--colour-by",
                             "DIAG", "--pair-lines", "--embeddings", "o/retrieval_embeddings.pt",
                             "-a", "resnet18", "--arch-version", "v32", "--amp", "--amp-dtype", "bf16",
                             "--retrieval-k", "1", "5", "--bootstrap", "2000"])  # backbone_retrieval's line is accepted
    assert (a.perplexity, a.map_iters, a.map_init, a.map_seed) == (12.5, 300, "pca", 9)
    assert a.colour_by == "DIAG" and a.pair_lines and a.embeddings == "o/retrieval_embeddings.pt" and a.arch == "resnet18"
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--colour-by", "age"])
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--map-init", "spectral"])


def test_backbone_map_refuses_before_the_device_is_touched(tmp_path, monkeypatch):
    bm = _tool("backbone_map")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("the device was touched")))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: (_ for _ in ()).throw(AssertionError("the device was touched")))
    syn = ["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "--log-path", str(tmp_path), "-b", "8", "--val-steps", "4",
           "--perplexity", "10"]
    for extra, text in ((["--perplexity", "0.5"], "perplexity"), (["--perplexity", "21.1"], "perplexity"),   # 64 points: <= 21
                        (["--map-iters", "0"], "iters"), (["--map-seed", "-1"], "seed"),
                        (["--colour-by", "DIAG"], "real dataset"), (["--val-steps", "1025"], "held-out cases"),   # 8200 cases
                        (["-b", "1", "--val-steps", "1"], "held-out cases"),
                        (["--embeddings", str(tmp_path / "missing.pt")], "does not exist"),
                        (["--pretrain-path", str(tmp_path / "none.pth")], "checkpoint")):
        with pytest.raises(SystemExit, match=text) as e:
            bm.main(syn + extra)
        assert e.value.code not in (0, None), extra
    with pytest.raises(SystemExit):
        bm.main(["--data-name", "synthetic", "--data-path", "-", "-a", "vgg16", "--log-path", str(tmp_path)])
    torch.save({"derm": torch.zeros(1, 4), "clinic": torch.zeros(1, 4)}, tmp_path / "one.pt")
    with pytest.raises(SystemExit, match="cases in --embeddings"):
        bm.main(syn + ["--embeddings", str(tmp_path / "one.pt")])
    torch.save({"other": 1}, tmp_path / "not.pt")
    with pytest.raises(SystemExit, match="is not a retrieval_embeddings.pt"):
        bm.main(syn + ["--embeddings", str(tmp_path / "not.pt")])
    torch.save({"derm": torch.zeros(6, 4), "clinic": torch.zeros(6, 4)}, tmp_path / "six.pt")
    with pytest.raises(SystemExit, match="perplexity"):                            # 12 points: at most 11 / 3
        bm.main(syn + ["--embeddings", str(tmp_path / "six.pt")])
    import shutil
    meta = os.path.join(ROOT, "tests", "golden", "derm7pt_meta")                   # a derm7pt tree without its images
    tree = tmp_path / "7PC"
    os.makedirs(tree / "images")
    for f in ("meta.csv", "train_indexes.csv", "valid_indexes.csv", "test_indexes.csv"):
        shutil.copy(os.path.join(meta, f), tree / f)
    real = ["--data-name", "SevenPCBaseDataset", "--data-path", str(tree), "-a", "resnet18", "--log-path", str(tmp_path)]
    with pytest.raises(SystemExit, match="checkpoint"):                            # real data needs a checkpoint
        bm.main(real)
    with pytest.raises(SystemExit, match="the test split"):                        # embeddings of other cases than the split's
        bm.main(real + ["--embeddings", str(tmp_path / "six.pt"), "--perplexity", "3"])
