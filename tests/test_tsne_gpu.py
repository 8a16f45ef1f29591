"""GPU: exact t-SNE maps (csrc/tsne.hip, sm3hip/tsne.py, tools/backbone_map.py) against the numpy restatement tests/tsne_ref.py.

  * distances: integer-valued x, |x| <= 8 (every partial sum is an integer below 2^24): D2 == the integer result, D2 == D2.T and
    a zero diagonal, for D in {1, 2, 3, 31, 32, 33, 128, 130} and N in {4, 5, 63, 64, 65, 129}; real inputs within
    (D + 2) 2^-24 relative of fp64 -- one rounding of the difference (counted twice: it is squared) and one per fma, all terms
    non-negative, so the bound is a derivation.
  * affinities for N in {5, 64, 65, 255, 256, 257, 600}, perplexities from {2, 30, (N - 1) / 3} where allowed, on Gaussian inputs
    at scales 1e-4, 1 and 1e4, ten exact duplicate pairs, one outlier at 1e3 times the scale, and an all-equal input.  All
    from the kernel's own D2: conditional rows within 2^-22 relative (4 x the fp32 storage rounding; absolute floor: fp32's
    least normal) of the restatement; every row's perplexity -- H of the restatement's row sums at the kernel's beta, so the
    fp32 storage of c does not enter -- within 1e-6 of the target (not for the all-equal input, whose rows have perplexity N - 1
    whatever beta is, nor for a row with more points tied at its least distance than the perplexity, which only the duplicate
    pairs produce); P == P.T; no NaN; the all-equal input gives exactly uniform rows.
  * forces for the same N with maps at scales 1e-4, 1 and 50, P from the affinities kernel: Z_i, A_i, R_i against the fp64
    restatement on the same fp32 map.  The fp32 roundings on a pair's path: dx, dy (2), the two fma of q (2), the division (1):
    5 for w, so 5 for Z; A = p w dx carries dx once more: 6; R = w w dx carries w twice and dx: 11.  (Each rounding moves its
    result by at most 2^-24 relative, and first-order every factor enters the term with weight <= 1 -- dx^2 / q <= 1.)  Allowed:
    2 x count x 2^-24 x the fp64 sum of the terms' absolute values; the fp64 accumulation is 2^-29 of that and is not counted.
  * one update step from the kernel's own F: update and y within 1 fp32 ulp of the restatement, gains equal wherever
    update g != 0, the gradient-norm sum within N 2^-52 relative.
  * KL within 1e-12 relative of the restatement evaluated with the kernel's pair arithmetic (fp32 w, widened).
  * tsne() is a function of its inputs: two runs, and a third after unrelated allocations and a map of another N, agree in
    every bit of map, history and beta.
  * end to end: the quality condition of tests/test_tsne_cpu.py on the GPU maps of seeds 0 .. 4 (N = 300, 1000 iterations).
  * tools/backbone_map.py on 32 synthetic cases writes map.csv / map.json / map.png; again from the saved embeddings: the same
    bytes of map.csv."""
import functools
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tsne_ref as R  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
NS = [5, 64, 65, 255, 256, 257, 600]
KINDS = ["gauss1e-4", "gauss1", "gauss1e4", "duplicates", "outlier", "equal"]
ROUNDINGS = {"Z": 5, "A": 6, "R": 11}


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CPU = _load("sm3_tsne_cpu_helpers", os.path.join(ROOT, "tests", "test_tsne_cpu.py"))  # quality_bounds, golden_input


def _gpu(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _sqdist(x):
    from sm3hip import ops
    d2 = torch.full((x.shape[0], x.shape[0]), float("nan"), dtype=torch.float32, device=DEV)
    ops.tsne_sqdist(_gpu(x, torch.float32), d2)
    return d2


# ---- distances ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4, 5, 63, 64, 65, 129])
def test_sqdist_is_exact_on_integers_and_within_the_derived_bound_on_reals(N):
    for D in (1, 2, 3, 31, 32, 33, 128, 130):
        rs = np.random.RandomState(1000 * N + D)
        x = rs.randint(-8, 9, (N, D)).astype(np.float32)
        x[N - 1] = x[0]                                                          # one exact duplicate: an off-diagonal zero
        got = _sqdist(x).cpu().numpy()
        xi = x.astype(np.int64)
        want = ((xi[:, None, :] - xi[None, :, :]) ** 2).sum(axis=2)
        assert np.array_equal(got, want.astype(np.float32)), (N, D)
        assert np.array_equal(got.view(np.uint32), got.T.view(np.uint32)) and not got.diagonal().any()
        x = (rs.randn(N, D) * 10.0 ** rs.randint(-2, 3)).astype(np.float32)
        got = _sqdist(x).cpu().numpy()
        want = R.sqdist(x)
        assert np.isfinite(got).all() and (np.abs(got - want) <= (D + 2) * U * want).all(), (N, D)
        assert np.array_equal(got.view(np.uint32), got.T.view(np.uint32)) and not got.diagonal().any()


# ---- affinities ---------------------------------------------------------------------------------------------------------
def make_x(N, kind):
    rs = np.random.RandomState(N)
    if kind == "equal":
        return np.full((N, 8), 0.37, dtype=np.float32)
    scale = {"gauss1e-4": 1e-4, "gauss1e4": 1e4}.get(kind, 1.0)
    x = rs.randn(N, 8) * scale
    if kind == "duplicates":
        for a in range(min(10, N // 2)):
            x[2 * a + 1] = x[2 * a]
    if kind == "outlier":
        x[N // 2] = 1e3 * scale * rs.randn(8)
    return x.astype(np.float32)


def perplexities(N):
    return [p for p in (2.0, 30.0, (N - 1) / 3) if 1.0 <= p <= (N - 1) / 3]


@functools.lru_cache(maxsize=2)
def _affinities(N, kind, perplexity):
    """The kernels' (d2, cond, beta, P) as numpy, every output pre-filled with NaN."""
    from sm3hip import ops
    d2 = _sqdist(make_x(N, kind))
    cond = torch.full((N, N), float("nan"), dtype=torch.float32, device=DEV)
    beta = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
    P = torch.full((N, N), float("nan"), dtype=torch.float32, device=DEV)
    ops.tsne_affinities(d2, perplexity, cond, beta)
    ops.tsne_symmetrise(cond, P)
    return d2.cpu().numpy(), cond.cpu().numpy(), beta.cpu().numpy(), P.cpu().numpy()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", NS)
def test_affinities_against_the_restatement(N, kind):
    tiny = float(np.finfo(np.float32).tiny)
    for perplexity in perplexities(N):
        d2, cond, beta, P = _affinities(N, kind, perplexity)
        assert np.isfinite(cond).all() and np.isfinite(beta).all() and np.isfinite(P).all() and (beta > 0).all()
        assert not cond.diagonal().any() and not P.diagonal().any()
        want, _ = R.conditional(d2, perplexity)
        err = np.abs(cond.astype(np.float64) - want)
        assert (err <= 2.0 ** -22 * want + tiny).all(), (N, kind, perplexity, float((err / (want + tiny)).max()))
        assert np.array_equal(P.view(np.uint32), P.T.view(np.uint32))
        assert np.array_equal(P, R.symmetrise(cond))
        if kind == "equal":
            uniform = np.where(np.eye(N, dtype=bool), np.float32(0), np.float32(1.0 / (N - 1)))
            assert np.array_equal(cond, uniform) and np.array_equal(beta, np.full(N, 2.0 ** 100))
        else:
            # a row with k points tied at its least distance has perplexity >= k whatever beta is: such rows (duplicates only) are
            # compared with the restatement above, the target is asked of all the others
            off = np.where(np.eye(N, dtype=bool), np.inf, d2)
            can = (off == off.min(axis=1, keepdims=True)).sum(axis=1) <= perplexity
            assert can.all() or kind == "duplicates"
            H, _, _ = R.row_entropy(d2, beta)
            at_beta = np.abs(np.exp(H) - perplexity)[can].max()
            stored = np.abs(R.row_perplexity(cond) - perplexity)[can].max()
            print(f"N {N} {kind} perplexity {perplexity:.4g}: rows {float((err / (want + tiny)).max()):.3g} relative, perplexity at beta "
                  f"{at_beta:.3g}, of the stored fp32 rows {stored:.3g}, {int((~can).sum())} rows cannot reach it")
            assert at_beta <= 1e-6, (N, kind, perplexity)


# ---- forces, update, KL -------------------------------------------------------------------------------------------------
def _map(N, scale):
    return (np.random.RandomState(7 * N).randn(N, 2) * scale).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _P(N):
    return _affinities(N, "gauss1", perplexities(N)[-1] if N < 100 else 30.0)[3]


def _forces(P, y):
    from sm3hip import ops
    F = torch.full((y.shape[0], 5), float("nan"), dtype=torch.float64, device=DEV)
    ops.tsne_forces(_gpu(P), _gpu(y), F)
    return F


@pytest.mark.parametrize("scale", [1e-4, 1.0, 50.0])
@pytest.mark.parametrize("N", NS)
def test_forces_within_the_counted_roundings(N, scale):
    P, y = _P(N), _map(N, scale)
    got = _forces(P, y).cpu().numpy()
    want, mass = R.forces(P, y), R.forces(P, y, absolute=True)
    assert np.isfinite(got).all()
    for name, cols in (("Z", [0]), ("A", [1, 2]), ("R", [3, 4])):
        err, allowed = np.abs(got[:, cols] - want[:, cols]), 2 * ROUNDINGS[name] * U * mass[:, cols]
        print(f"N {N} scale {scale:g} {name}: {float((err / (U * mass[:, cols])).max()):.3g} u of {2 * ROUNDINGS[name]} u allowed")
        assert (err <= allowed).all(), (N, scale, name)


@pytest.mark.parametrize("N", NS)
def test_one_update_step_and_the_kl(N):
    from sm3hip import ops
    rs = np.random.RandomState(N + 1)
    P, y = _P(N), _map(N, 1.0)
    upd = (rs.randn(N, 2) * 0.1).astype(np.float32)
    upd[0] = 0.0                                                                 # update g == 0: the sign is not asked
    gains = (0.005 + rs.rand(N, 2) * 2.0).astype(np.float32)
    Fd = _forces(P, y)
    F = Fd.cpu().numpy()
    # KL first: it reads the map before the step moves it
    rows = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
    res = torch.full((2, 2), float("nan"), dtype=torch.float64, device=DEV)
    ops.tsne_kl(_gpu(P), _gpu(y), Fd, rows, res[0])
    want_kl = R.kl(P, y, F, arithmetic="fp32")
    got_kl, got_z = (float(v) for v in res[0].cpu())
    assert got_z == R.fixed_sum(F[:, 0])
    assert abs(got_kl - want_kl) <= 1e-12 * abs(want_kl), (got_kl, want_kl)
    for e, m in ((12.0, 0.5), (1.0, 0.8)):
        yd, ud, gd = _gpu(y), _gpu(upd), _gpu(gains)
        ops.tsne_update(Fd, e, m, 200.0, yd, ud, gd, res[1])
        y1, u1, g1, g, gn2, Z = R.update(F, e, m, 200.0, y, upd, gains)
        got_gn2, got_z = (float(v) for v in res[1].cpu())
        assert got_z == Z
        assert (np.abs(ud.cpu().numpy() - u1) <= np.spacing(np.abs(u1))).all()
        assert (np.abs(yd.cpu().numpy() - y1) <= np.spacing(np.abs(y1))).all()
        asked = upd.astype(np.float64) * g != 0
        assert asked.sum() == 2 * N - 2 and np.array_equal(gd.cpu().numpy()[asked], g1[asked])
        assert (gd.cpu().numpy() >= np.float32(0.01)).all()
        assert abs(got_gn2 - gn2) <= N * 2.0 ** -52 * gn2, (got_gn2, gn2)


# ---- the whole map ------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.numpy().view(np.uint8), b.numpy().view(np.uint8))


def test_tsne_is_a_function_of_its_inputs():
    from sm3hip import tsne
    x = _gpu(CPU.golden_input()[0])
    kw = dict(perplexity=20.0, iters=400, exaggeration_iters=150, seed=3)
    first = tsne.tsne(x, **kw)
    again = tsne.tsne(x.clone(), **kw)
    junk = [torch.randn(n, 7, device=DEV) for n in (1000, 33, 4097)]             # move the allocator
    other = tsne.tsne(_gpu(make_x(130, "gauss1")), perplexity=9.0, iters=60, exaggeration_iters=20, check_every=10)
    third = tsne.tsne(x, **kw)
    del junk
    assert len(first["history"]) == 8 and first["iters_run"] == 400 and len(other["history"]) == 6
    for rep in (again, third):
        assert _same(rep["map"], first["map"]) and _same(rep["beta"], first["beta"])
        assert rep["history"] == first["history"] and rep["kl"] == first["kl"]
    assert np.isfinite(first["map"].numpy()).all() and first["history"][-1][1] < first["history"][0][1]
    moved = tsne.tsne(x, **{**kw, "seed": 4})
    assert not _same(moved["map"], first["map"]) and _same(moved["beta"], first["beta"])
    pca = tsne.tsne(x, **{**kw, "init": "pca"})
    given = tsne.tsne(x, **{**kw, "init": tsne.pca_init(x).numpy()})
    assert _same(pca["map"], given["map"]) and pca["init"] == "pca" and given["init"] == "array"
    assert first["learning_rate"] == 50.0 and tsne.tsne(x, **{**kw, "iters": 1, "learning_rate": 10})["learning_rate"] == 10.0


def test_affinities_and_return_p():
    from sm3hip import tsne
    x = _gpu(CPU.golden_input()[0])
    aff = tsne.affinities(x, 30.0)
    rep = tsne.tsne(x, iters=2, return_p=True)
    assert sorted(aff) == ["P", "beta", "sqdist"] and torch.equal(aff["P"], rep["P"])
    assert torch.equal(aff["beta"].cpu(), rep["beta"]) and torch.equal(aff["P"], aff["P"].T)
    assert abs(float(aff["P"].double().sum()) - 1.0) < 1e-6


def test_end_to_end_quality_condition():
    from sm3hip import tsne
    kl_max, tw_min, _ = CPU.quality_bounds()
    x, _ = CPU.golden_input()
    xd = _gpu(x)
    for seed in CPU.SEEDS:
        rep = tsne.tsne(xd, seed=seed)
        tw = R.trustworthiness(x, rep["map"].numpy(), 10)
        print(f"seed {seed}: KL {rep['kl']:.5f} (<= {kl_max:.5f}), trustworthiness {tw:.5f} (>= {tw_min:.5f})")
        assert rep["iters_run"] == 1000 and len(rep["history"]) == 20
        assert rep["kl"] <= kl_max and tw >= tw_min, (seed, rep["kl"], tw)


def test_cross_modal_map():
    from sm3hip import tsne
    x, _ = CPU.golden_input()
    derm = _gpu(x[:150])
    clinic = _gpu(x[:150] + np.float32(0.05) * np.random.RandomState(5).randn(150, 16).astype(np.float32))
    rep = tsne.cross_modal_map(derm, clinic, perplexity=20.0, iters=500)
    both = tsne.tsne(torch.cat([derm, clinic]), perplexity=20.0, iters=500)
    assert _same(torch.cat([rep["derm"], rep["clinic"]]), both["map"]) and rep["tsne"]["kl"] == both["kl"]
    assert rep["partner_rank"].shape == (150, 2) and rep["partner_rank"].min() >= 1 and rep["partner_rank"].max() <= 299
    assert torch.equal(rep["partner_rank"], tsne.partner_ranks(rep["derm"], rep["clinic"]))
    print(f"median partner rank {rep['median_partner_rank']}, preservation {rep['preservation']:.4f}")
    # a partner is 0.2 away where a neighbour of the same island is about 5.7 away: it stays among the 10 nearest of the map,
    # which alone is three times the 10 / 299 of a map that knows nothing
    assert rep["median_partner_rank"] <= 10 and 0.1 < rep["preservation"] <= 1.0 and rep["k"] == 10


# ---- the tool -----------------------------------------------------------------------------------------------------------
def test_backbone_map_writes_its_files_and_repeats_from_the_saved_embeddings(tmp_path, capsys):
    from PIL import Image
    bm = _load("sm3_tsne_gpu_backbone_map", os.path.join(TOOLS, "backbone_map.py"))
    base = ["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "--arch-version", "v32", "-b", "8", "--val-steps", "4",
            "--img-sz", "64", "64", "--amp", "--amp-dtype", "bf16", "--perplexity", "10", "--map-iters", "300"]
    out = bm.main(base + ["--save-embeddings", "--pair-lines", "--log-path", str(tmp_path / "a")])
    text = capsys.readouterr().out
    assert text.count("map N=32 cases (64 points): KL ") == 1
    for f in ("map.csv", "map.json", "map.png", "retrieval_embeddings.pt"):
        assert os.path.isfile(tmp_path / "a" / f), f
    rows = [l.split(",") for l in open(tmp_path / "a" / "map.csv").read().splitlines()]
    assert rows[0][:4] == ["case", "modality", "x", "y"] and len(rows[0]) == 12 and len(rows) == 65
    assert [r[1] for r in rows[1:]] == ["derm"] * 32 + ["clinic"] * 32 and [int(r[0]) for r in rows[1:33]] == list(range(32))
    xy = np.array([[float(r[2]), float(r[3])] for r in rows[1:]], dtype=np.float32)
    assert np.array_equal(xy, torch.cat([out["map"]["derm"], out["map"]["clinic"]]).numpy())   # repr parses back exactly
    assert all(v == "" for r in rows[1:] for v in r[4:])                             # synthetic cases have no labels
    saved = json.load(open(tmp_path / "a" / "map.json"))
    assert saved["cases"] == 32 and saved["N"] == 64 and saved["kl"] == out["map"]["tsne"]["kl"] and saved["iters_run"] == 300
    assert len(saved["history"]) == 6 and saved["k"] == 10 and 0 <= saved["preservation"] <= 1 and saved["median_partner_rank"] >= 1
    im = Image.open(tmp_path / "a" / "map.png")
    assert im.size == (1024, 1024) and im.format == "PNG"
    bm.main(base + ["--embeddings", str(tmp_path / "a" / "retrieval_embeddings.pt"), "--log-path", str(tmp_path / "b")])
    assert open(tmp_path / "b" / "map.csv", "rb").read() == open(tmp_path / "a" / "map.csv", "rb").read()
    assert not os.path.exists(tmp_path / "b" / "retrieval_embeddings.pt")
