"""CPU: deletion / insertion faithfulness curves (sm3hip/faith.py, csrc/faith.hip) -- the entry points in the header, the
binding and the library and their host-side refusals; the numpy restatements of the two kernels (ranks, counts, compose) that
tests/test_faith_gpu.py compares the device against bit for bit, checked here against the O(HW^2) definition and a stable
argsort; the torch restatement of the curves (any dtype: float64 is the reference, float32 the yardstick) on a hand-computable
linear model; the trapezoid; the driver's and the two tools' refusals (each before anything touches the GPU)."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]
ENTRY_POINTS = ("sm3_faith_rank", "sm3_faith_rank_workspace", "sm3_faith_compose")


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ATTR = _load("sm3_faith_attr_ref", os.path.join(ROOT, "tests", "test_attr_cpu.py"))  # the linear model


# ---- numpy restatements of the kernels (used by tests/test_faith_gpu.py) -------------------------------------------------
def ranks(maps):
    """sm3_faith_rank: maps [..., HW] f32 -> int32 ranks [..., HW]; per row descending by value (IEEE: -0 == +0), ties by
    ascending index.  A stable argsort of the negated values: negation is exact and turns -0 / +0 into +0 / -0, equal again."""
    m = np.ascontiguousarray(maps, dtype=np.float32)
    flat = m.reshape(-1, m.shape[-1])
    out = np.empty(flat.shape, np.int32)
    idx = np.arange(flat.shape[1], dtype=np.int32)
    for r, row in enumerate(flat):
        out[r, np.argsort(-row, kind="stable")] = idx
    return out.reshape(m.shape)


def ranks_by_definition(row):
    """rank[p] = #{q : map[q] > map[p]} + #{q < p : map[q] == map[p]}, O(HW^2)."""
    row = np.asarray(row, np.float32)
    gt = (row[None, :] > row[:, None]).sum(1)
    eq = np.tril(row[None, :] == row[:, None], -1).sum(1)
    return (gt + eq).astype(np.int32)


def counts(HW, S):
    """c_k = (k * HW) // S, k = 0 .. S, in Python integers."""
    return [(k * HW) // S for k in range(S + 1)]


def compose(x, base, rk, k0, c, steps, invert):
    """sm3_faith_compose: x [N, 3, HW], base [1 | N, 3, HW], rk [N, T, HW] -> out [c, T, N, 3, HW]: base where (rank < c_k) !=
    invert, else x.  Pure selection: bit copies."""
    N, _, HW = x.shape
    T = rk.shape[1]
    ck = counts(HW, steps)
    b = np.broadcast_to(base, x.shape)
    out = np.empty((c, T, N, 3, HW), np.float32)
    for j in range(c):
        sel = (rk < ck[k0 + j]) != bool(invert)                       # [N, T, HW]
        out[j] = np.where(sel.transpose(1, 0, 2)[:, :, None, :], b[None], x[None])
    return out


# ---- the torch restatement of the curves (float64: the reference; float32: the yardstick) --------------------------------
def ref_deletion_insertion(fn, derm, clinic, base_d, base_c, rk, tc, steps, modality="joint"):
    """Both curves in the dtype of the inputs.  fn(derm, clinic) -> 8 logits [M, n_i]; rk [N, 8, 2, H, W] integer ranks; tc
    [N, 8].  Step k of label t perturbs the pixels with rank < c_k (deletion: to the baseline; insertion: every other pixel is
    the baseline).  Returns {"deletion", "insertion": [N, 8, S + 1] float64 probabilities softmax(logits_t.double())[tc],
    "deletion_logit", "insertion_logit": the target logits themselves, in fn's dtype, "deletion_auc", "insertion_auc"}."""
    N, _, H, W = derm.shape
    T, HW = len(NUM_CLASSES), H * W
    xs, bs = [derm, clinic], [base_d.expand_as(derm), base_c.expand_as(clinic)]
    ck = counts(HW, steps)
    pert = [m for m, name in enumerate(("derm", "clinic")) if modality in ("joint", name)]
    out = {}
    with torch.no_grad():
        for name, invert in (("deletion", False), ("insertion", True)):
            prob = torch.empty(N, T, steps + 1, dtype=torch.float64)
            logit = torch.empty(N, T, steps + 1, dtype=derm.dtype)
            for k in range(steps + 1):
                ins = []
                for m in range(2):
                    if m in pert:
                        sel = ((rk[:, :, m] < ck[k]) != invert).permute(1, 0, 2, 3)[:, :, None]        # [T, N, 1, H, W]
                        ins.append(torch.where(sel, bs[m][None], xs[m][None]).reshape(T * N, 3, H, W))
                    else:
                        ins.append(xs[m].repeat(T, 1, 1, 1))
                logits = fn(ins[0], ins[1])
                for t in range(T):
                    lg = logits[t][t * N:(t + 1) * N]
                    logit[:, t, k] = lg.gather(1, tc[:, t:t + 1])[:, 0]
                    prob[:, t, k] = torch.softmax(lg.double(), dim=1).gather(1, tc[:, t:t + 1])[:, 0]
            out[name], out[name + "_logit"], out[name + "_auc"] = prob, logit, trapezoid(prob)
    return out


def trapezoid(curve):
    """(p_0 / 2 + p_1 + ... + p_{S-1} + p_S / 2) / S in float64, ascending k."""
    c = curve.double()
    S = c.shape[-1] - 1
    acc = c[..., 0] / 2
    for k in range(1, S):
        acc = acc + c[..., k]
    return (acc + c[..., S] / 2) / S


# ---- the restatements against the definition ----------------------------------------------------------------------------
def test_ranks_equal_the_definition_on_ties_signed_zeros_negatives_and_constants():
    got = ranks(np.float32([0.0, -0.0, 1.0, 0.0, -0.0, 1.0, -1.0]))
    assert got.tolist() == [2, 3, 0, 4, 5, 1, 6]
    g = np.random.default_rng(0)
    cases = [g.standard_normal(64), np.round(g.standard_normal(200) * 1.5), np.zeros(16), np.full(9, -2.5),
             g.integers(0, 4, 300) / 4.0, np.float32([3, -0.0, 0.0, -3, 1e-45, -1e-45, 3e38, -3e38, 1e-45, 0.0]),
             np.where(g.random(128) < 0.5, 0.0, 1.0), np.float32([5.0]), -np.abs(g.standard_normal(50))]
    for row in cases:
        row = np.float32(row)
        r = ranks(row)
        assert r.dtype == np.int32 and np.array_equal(r, ranks_by_definition(row))
        assert sorted(r.tolist()) == list(range(row.size))                       # a permutation
        order = np.argsort(-row, kind="stable")
        assert np.array_equal(r[order], np.arange(row.size))
        assert np.all(np.diff(row[order]) <= 0)                                  # descending by value
    m = np.float32(g.integers(-2, 3, (2, 3, 40)))
    assert np.array_equal(ranks(m)[1, 2], ranks_by_definition(m[1, 2])) and ranks(m).shape == m.shape


def test_counts_and_compose_by_hand():
    assert counts(8, 4) == [0, 2, 4, 6, 8] and counts(10, 4) == [0, 2, 5, 7, 10] and counts(4, 4) == [0, 1, 2, 3, 4]
    assert counts(50176, 32)[1] == 1568 and counts(7, 1) == [0, 7]
    for HW, S in ((50176, 32), (1028, 7), (4096, 4096), (200704, 1000)):
        c = counts(HW, S)
        assert c[0] == 0 and c[-1] == HW and all(b > a for a, b in zip(c, c[1:]))
    from sm3hip.faith import counts as lib_counts
    assert lib_counts(1028, 7) == counts(1028, 7)
    x = np.arange(1, 13, dtype=np.float32).reshape(1, 3, 4)
    b = -np.ones((1, 3, 4), np.float32)
    rk = np.int32([[[2, 0, 3, 1], [0, 1, 2, 3]]])                                # N = 1, T = 2
    out = compose(x, b, rk, 0, 3, 2, 0)                                          # S = 2: c_k = 0, 2, 4
    assert out.shape == (3, 2, 1, 3, 4)
    assert np.array_equal(out[0, 0, 0], x[0]) and np.array_equal(out[2, 1, 0], b[0])
    assert np.array_equal(out[1, 0, 0, 0], np.float32([1, -1, 3, -1])) and np.array_equal(out[1, 1, 0, 2], np.float32([-1, -1, 11, 12]))
    ins = compose(x, b, rk, 1, 1, 2, 1)
    assert np.array_equal(ins[0, 0, 0, 1], np.float32([-1, 6, -1, 8]))


def _linear_case(seed, hw=4):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    ws = [(rnd(n, 3, hw, hw), rnd(n, 3, hw, hw)) for n in NUM_CLASSES]
    derm, clinic = rnd(2, 3, hw, hw), rnd(2, 3, hw, hw)
    tc = torch.stack([torch.randint(0, n, (2,), generator=g) for n in NUM_CLASSES], dim=1)
    # the map = each pixel's contribution to the target logit (summed over the channels)
    maps = torch.stack([torch.stack([(x * w[m][tc[:, t]]).sum(1) for m, x in enumerate((derm, clinic))], dim=1)
                        for t, w in enumerate(ws)], dim=1)
    return ws, derm, clinic, tc, maps, g


@pytest.mark.parametrize("modality", ["joint", "derm", "clinic"])
def test_restatement_on_a_linear_model_true_ranking_deletes_fastest(modality):
    """logit = sum(w x) + 1/4 with w, x >= 0 and a zero baseline: deleting a pixel removes its contribution, so after c_k
    pixels the logit under the ranking by contribution is the lowest any order of c_k pixels can reach."""
    ws, derm, clinic, tc, maps, g = _linear_case(3)
    fn = ATTR._linear_fn(ws)
    zero = torch.zeros(1, 3, 4, 4, dtype=torch.float64)
    S = 8
    true = torch.from_numpy(ranks(maps.float().numpy()))
    rev = 15 - true
    rnd = torch.stack([torch.randperm(16, generator=g) for _ in range(2 * 8 * 2)]).view(2, 8, 2, 4, 4).int()
    run = lambda rk: ref_deletion_insertion(fn, derm, clinic, zero, zero, rk, tc, S, modality)
    a, b, c = run(true), run(rev), run(rnd)
    assert a["deletion"].shape == (2, 8, S + 1) and a["deletion"].dtype == torch.float64
    assert bool((a["deletion_logit"] <= b["deletion_logit"] + 1e-12).all())
    assert bool((a["deletion_logit"] <= c["deletion_logit"] + 1e-12).all())
    assert bool((a["insertion_logit"] >= c["insertion_logit"] - 1e-12).all())
    assert float((b["deletion_logit"] - a["deletion_logit"]).max()) > 0.1
    # the end points are the two logits
    at = lambda d, c_: torch.stack([o.gather(1, tc[:, t:t + 1])[:, 0] for t, o in enumerate(fn(d, c_))], dim=1)
    zd, zc = torch.zeros_like(derm), torch.zeros_like(clinic)
    end = at(zd if modality != "clinic" else derm, zc if modality != "derm" else clinic)
    for r in (a, b, c):
        assert torch.allclose(r["deletion_logit"][:, :, 0], at(derm, clinic), rtol=0, atol=1e-12)
        assert torch.allclose(r["insertion_logit"][:, :, S], at(derm, clinic), rtol=0, atol=1e-12)
        assert torch.allclose(r["deletion_logit"][:, :, S], end, rtol=0, atol=1e-12)
        assert torch.allclose(r["insertion_logit"][:, :, 0], end, rtol=0, atol=1e-12)
    if modality == "joint":
        assert torch.allclose(end, torch.full_like(end, 0.25))
    # the logit curve by hand for one (image, label): the bias and the contributions that are left
    n, t = 1, 4
    cd, cc = maps[n, t, 0].reshape(-1), maps[n, t, 1].reshape(-1)
    rd, rc = true[n, t, 0].reshape(-1), true[n, t, 1].reshape(-1)
    for k, ck in enumerate(counts(16, S)):
        want = 0.25 + (cd[rd >= ck].sum() if modality != "clinic" else cd.sum()) + (cc[rc >= ck].sum() if modality != "derm" else cc.sum())
        assert abs(float(a["deletion_logit"][n, t, k] - want)) < 1e-12


def test_trapezoid_and_the_library_auc_agree():
    from sm3hip.faith import auc
    c = torch.tensor([[1.0, 0.5, 0.25, 0.0], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]], dtype=torch.float64)
    want = torch.tensor([(0.5 + 0.5 + 0.25 + 0.0) / 3, 0.0, 1.0], dtype=torch.float64)
    assert torch.equal(trapezoid(c), want) and torch.equal(auc(c), want)
    g = torch.Generator().manual_seed(1)
    r = torch.rand(2, 8, 33, generator=g, dtype=torch.float64)
    assert torch.equal(auc(r), trapezoid(r)) and auc(r).shape == (2, 8) and auc(r).dtype == torch.float64
    assert torch.equal(auc(r[..., :2]), (r[..., 0] / 2 + r[..., 1] / 2))         # S = 1
    with pytest.raises(ValueError):
        auc(r[..., :1])


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def _lib():
    from sm3hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_entry_points_are_declared_bound_and_exported():
    from sm3hip import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sm3_hip.h")).read(), flags=re.S)
    lib = _lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text)
        assert name in L.SIGNATURES
        assert hasattr(lib, name)
    assert lib.sm3_abi_version() == 9  # additive: the version stays
    from sm3hip import faith, ops
    assert callable(faith.deletion_insertion) and callable(ops.faith_rank) and callable(ops.faith_compose)
    assert "faith.hip" in open(os.path.join(ROOT, "skin-sm3_amd", "csrc", "Makefile")).read()


def _p(v):
    return C.c_void_p(v) if v else C.c_void_p(0)


def _rank(lib, maps=0x1000, ranks=0x2000, rows=2, HW=64, ws=0x3000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(lib.sm3_faith_rank_workspace(rows, HW), 0)
    return lib.sm3_faith_rank(_p(maps), _p(ranks), rows, HW, _p(ws), ws_bytes, C.c_void_p(0))


def _compose(lib, x=0x1000, base=0x2000, base_n=1, ranks=0x3000, sn=1024, st=128, out=0x4000, N=2, T=8, HW=64, k0=0, c=4,
             steps=8, invert=0):
    return lib.sm3_faith_compose(_p(x), _p(base), base_n, _p(ranks), sn, st, _p(out), N, T, HW, k0, c, steps, invert,
                                 C.c_void_p(0))


@pytest.mark.parametrize("kw,code", [
    (dict(maps=0), -1), (dict(ranks=0), -1), (dict(ws=0), -1), (dict(rows=0), -1), (dict(HW=0), -1), (dict(rows=-3), -1),
    (dict(HW=2 ** 24 + 1, ws_bytes=2 ** 40), -1), (dict(rows=2 ** 16, HW=2 ** 16, ws_bytes=2 ** 40), -1),
    (dict(ws_bytes=2 * 2 * 64 * 8 - 1), -1), (dict(ws_bytes=0), -1),
    (dict(maps=0x1002), -2), (dict(ranks=0x2001), -2), (dict(ws=0x3004), -2)])
def test_rank_rejects_bad_arguments_before_any_launch(kw, code):
    assert _rank(_lib(), **kw) == code, kw


def test_rank_workspace_is_two_buffers_of_pairs_per_map():
    lib = _lib()
    assert lib.sm3_faith_rank_workspace(1, 4) == 64
    assert lib.sm3_faith_rank_workspace(128, 224 * 224) == 128 * 2 * 224 * 224 * 8
    assert lib.sm3_faith_rank_workspace(1, 448 * 448) == 2 * 448 * 448 * 8
    for rows, HW in ((0, 4), (4, 0), (-1, 4), (1, 2 ** 24 + 1), (1024, 448 * 448)):  # the last: past 2^31 - 1 bytes
        assert lib.sm3_faith_rank_workspace(rows, HW) == -1, (rows, HW)


@pytest.mark.parametrize("kw,code", [
    (dict(x=0), -1), (dict(base=0), -1), (dict(ranks=0), -1), (dict(out=0), -1), (dict(N=0), -1), (dict(T=0), -1),
    (dict(HW=0), -1), (dict(c=0), -1), (dict(steps=0), -1), (dict(k0=-1), -1), (dict(base_n=3), -1), (dict(invert=2), -1),
    (dict(invert=-1), -1), (dict(steps=65), -1), (dict(k0=6, c=4, steps=8), -1), (dict(k0=9, c=1, steps=8), -1),
    (dict(N=2 ** 10, T=2 ** 10), -1), (dict(sn=-4), -1), (dict(st=-4), -1), (dict(HW=2 ** 24 + 4), -1),
    (dict(HW=66), -2), (dict(x=0x1004), -2), (dict(base=0x2008), -2), (dict(ranks=0x3004), -2), (dict(out=0x4008), -2),
    (dict(sn=1026), -2), (dict(st=130), -2)])
def test_compose_rejects_bad_arguments_before_any_launch(kw, code):
    assert _compose(_lib(), **kw) == code, kw


# ---- the driver's host logic ------------------------------------------------------------------------------------------------
def test_driver_refuses_bad_arguments_before_touching_a_device():
    from sm3hip.faith import deletion_insertion as di
    from src.models.baseline import Baseline
    who = "deletion_insertion"
    m = Baseline("resnet18", None)
    x = torch.zeros(2, 3, 32, 32)
    maps = torch.rand(2, 8, 2, 32, 32)
    with pytest.raises(ValueError, match=who + ".*eval mode"):
        di(m.train(), x, x, maps)
    m.eval()
    with pytest.raises(ValueError, match=who + ".*CUDA tensor"):
        di(m, x, x, maps)
    with pytest.raises(TypeError, match="Baseline"):
        di(torch.nn.Linear(2, 2), x, x, maps)
    for bad in (maps[:, :7], maps[:, :, :1], maps[..., :16], maps.double(), maps.half(), maps[0], "maps", None):
        with pytest.raises(ValueError, match=who + ".*maps must be"):
            di(m, x, x, bad)
    for v in (float("nan"), float("inf"), float("-inf")):
        poisoned = maps.clone()
        poisoned[1, 3, 1, 5, 7] = v
        with pytest.raises(ValueError, match="finite"):
            di(m, x, x, poisoned)
    for steps in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="steps"):
            di(m, x, x, maps, steps=steps)
    for chunk in (0, 9, -1, 1.5):
        with pytest.raises(ValueError, match="chunk"):
            di(m, x, x, maps, steps=8, chunk=chunk)
    with pytest.raises(ValueError, match="mode"):
        di(m, x, x, maps, mode="all")
    with pytest.raises(ValueError, match="modality"):
        di(m, x, x, maps, modality="both")
    with pytest.raises(ValueError, match="baseline"):
        di(m, x, x, maps, baseline="black")


def test_wrappers_refuse_host_tensors_and_mismatched_shapes():
    from sm3hip import ops
    m, r = torch.rand(3, 64), torch.zeros(3, 64, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        ops.faith_rank(m, r)
    x, out = torch.zeros(2, 3, 8, 8), torch.zeros(4, 8, 2, 3, 8, 8)
    with pytest.raises(ValueError, match="GPU"):
        ops.faith_compose(x, x[:1], torch.zeros(2, 8, 8, 8, dtype=torch.int32), out, 0, 8, False)


def test_driver_refuses_sizes_the_kernels_do_not_take():
    from sm3hip.faith import deletion_insertion as di
    from src.models.baseline import Baseline
    m = Baseline("resnet18", None).eval()
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(ValueError, match="at most H \\* W"):
        di(m, x, x, torch.rand(1, 8, 2, 4, 4), steps=17)
    y = torch.zeros(1, 3, 3, 5)
    with pytest.raises(ValueError, match="multiple of 4"):
        di(m, y, y, torch.rand(1, 8, 2, 3, 5), steps=4)


# ---- the tools ----------------------------------------------------------------------------------------------------------
def _tool(name):
    return _load(f"sm3_{name}_cpu", os.path.join(TOOLS, f"{name}.py"))


def test_backbone_faith_parser_takes_the_cam_and_attr_lines_with_the_curve_flags():
    bf = _tool("backbone_faith")
    a = bf.get_parser().parse_args(["--data-path", "-", "--data-name", "synthetic"])
    assert (a.method, a.cam_layer, a.steps, a.samples, a.sigma, a.squared, a.attr_seed, a.chunk, a.target, a.split, a.max_cases,
            a.linear_path, a.arch, a.curve_steps, a.curve_mode, a.modality) == (
        "cam", "layer4", 32, 16, 0.15, False, 0, None, "pred", "test", 64, None, "resnet50", 32, "both", "joint")
    a = bf.get_parser().parse_args(["--data-path", "x", "--data-name", "SevenPCBaseDataset", "--method", "random",
                                    "--attr-seed", "9", "--chunk", "2", "--curve-steps", "16", "--curve-mode", "deletion",
                                    "--modality", "derm", "--target", "cls", "--split", "valid", "--max-cases", "5",
                                    "--linear-path", "p.pth", "-a", "resnet18", "--img-sz", "64", "96", "--amp", "--amp-dtype",
                                    "bf16"])
    assert (a.method, a.attr_seed, a.chunk, a.curve_steps, a.curve_mode, a.modality, a.target, a.split, a.max_cases,
            a.linear_path, a.arch, a.img_sz) == ("random", 9, 2, 16, "deletion", "derm", "cls", "valid", 5, "p.pth", "resnet18",
                                                 [64, 96])


def test_mlc_faith_parser_takes_the_cam_and_attr_lines_with_the_curve_flags():
    mf = _tool("mlc_faith")
    a = mf.get_parser().parse_args(["--data-path", "-", "--data-name", "synthetic"])
    assert (a.checkpoint, a.method, a.cam_layer, a.steps, a.curve_steps, a.mlc_proj, a.arch, a.test_sz, a.log_path) == (
        None, "cam", "layer4", 32, 32, "v4", "resnet50", 224, "./logs/mlc_faith")
    a = mf.get_parser().parse_args(["--data-path", "-", "--data-name", "synthetic", "--checkpoint", "c.pth", "--mlc-proj", "v2",
                                    "--mlc-proj-dim", "512", "--sa-dim-ff", "128", "--method", "ig", "--steps", "16",
                                    "--test-sz", "96", "--target", "cls", "--l2-norm", "--chunk", "4", "--curve-steps", "8",
                                    "--modality", "clinic"])
    assert (a.checkpoint, a.mlc_proj, a.mlc_proj_dim, a.steps, a.test_sz, a.target, a.l2_norm, a.chunk, a.curve_steps,
            a.modality) == ("c.pth", "v2", 512, 16, 96, "cls", True, 4, 8, "clinic")


@pytest.fixture
def no_gpu(monkeypatch):
    """Anything that reaches for the device fails the test."""
    def boom(*a, **k):
        raise AssertionError("touched the GPU before refusing")
    monkeypatch.setattr(torch, "Generator", boom)
    monkeypatch.setattr(torch.cuda, "synchronize", boom)
    monkeypatch.setattr(torch.nn.Module, "to", boom)
    from sm3hip import attr, cam, faith
    monkeypatch.setattr(attr, "integrated_gradients", boom)
    monkeypatch.setattr(attr, "smooth_grad", boom)
    monkeypatch.setattr(cam, "grad_cam", boom)
    monkeypatch.setattr(faith, "deletion_insertion", boom)


FAITH_REFUSALS = [
    (["--method", "occlusion"], "method"),
    (["--max-cases", "0"], "max-cases"),
    (["--curve-steps", "0"], "curve-steps"),
    (["--curve-steps", "8", "--chunk", "9"], "chunk"),
    (["--chunk", "0"], "chunk"),
    (["--curve-mode", "all"], "curve-mode"),
    (["--modality", "both"], "modality"),
    (["--method", "cam", "--cam-layer", "layer5"], "cam-layer"),
    (["--method", "ig", "--steps", "0"], "steps"),
    (["--method", "smoothgrad", "--samples", "0"], "samples"),
    (["--method", "smoothgrad", "--sigma", "-1"], "sigma"),
    (["--method", "random", "--attr-seed", "-1"], "attr-seed"),
]


@pytest.mark.parametrize("argv,msg", FAITH_REFUSALS + [
    (["--linear-path", "/nonexistent/best_linear.pth"], "does not exist"),
    (["-a", "resnext50_32x4d"], "not supported"),
    (["--img-sz", "3", "5"], "multiple of 4"),
    (["--img-sz", "4", "4", "--curve-steps", "17"], "curve-steps"),
])
def test_backbone_faith_refusals_stop_before_any_kernel(argv, msg, no_gpu, tmp_path):
    bf = _tool("backbone_faith")
    with pytest.raises(SystemExit, match=msg):
        bf.main(["--data-name", "synthetic", "--data-path", "-"] + argv + ["--log-path", str(tmp_path)])


@pytest.mark.parametrize("argv,msg", FAITH_REFUSALS + [
    (["--checkpoint", "/nonexistent/best_finetune.pth"], "does not exist"),
    (["-a", "resnet18"], "not supported"),
    (["--mlc-proj", "v9"], "mlc-proj"),
    (["--mlc-proj", "v0", "--mlc-proj-dim", "512"], "v0"),
    (["--test-sz", "7"], "multiple of 4"),
])
def test_mlc_faith_refusals_stop_before_any_kernel(argv, msg, no_gpu, tmp_path):
    mf = _tool("mlc_faith")
    with pytest.raises(SystemExit, match=msg):
        mf.main(["--data-name", "synthetic", "--data-path", "-"] + argv + ["--log-path", str(tmp_path)])


@pytest.mark.parametrize("tool,flag", [("backbone_faith", "linear-path"), ("mlc_faith", "checkpoint")])
def test_real_data_needs_weights(tool, flag, no_gpu, tmp_path):
    root = tmp_path / "7PC"
    os.makedirs(root / "images")
    for f in ("meta.csv", "train_indexes.csv", "valid_indexes.csv", "test_indexes.csv"):
        (root / f).write_text("")
    with pytest.raises(SystemExit, match=flag):
        _tool(tool).main(["--data-name", "SevenPCBaseDataset", "--data-path", str(root), "--log-path", str(tmp_path)])


@pytest.mark.parametrize("tool", ["backbone_faith", "mlc_faith"])
def test_unknown_data_is_refused(tool, no_gpu, tmp_path):
    with pytest.raises(SystemExit, match="not available"):
        _tool(tool).main(["--data-name", "ImageNet", "--data-path", "-", "--log-path", str(tmp_path)])
