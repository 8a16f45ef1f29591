"""CPU: the cross-modal retrieval report (sm3hip/retrieval.py, csrc/retrieval.hip, tools/backbone_retrieval.py).

  * the plain-numpy restatements the GPU tests compare the kernels with: beats(S), pack(b), counts(b, m, ks), loss_terms(S, tau),
    and the shared integer-valued inputs make_inputs(N, kind) (S exact, ties real); the table of the inputs' properties;
  * values_from_counts on hand-made counts: R@k, 1 + R / N, Q / (N 2^32) against fractions.Fraction within 2^-32, the median of
    even and odd N;
  * every host refusal, with no device; header, binding and the built library carry both symbols; the entry points refuse bad
    arguments before any launch;
  * the tools' parsers and their refusals before the device is touched; backbone_train's --retrieval-freq defaults to 0."""
import ctypes as C
import importlib.util
import os
import re
from fractions import Fraction

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


REPORT_REF = _load("sm3_retrieval_report_ref", os.path.join(ROOT, "tests", "test_report_cpu.py"))
multiplicities = REPORT_REF.multiplicities


# ---- the restatement ----------------------------------------------------------------------------------------------------
def make_inputs(N, kind, seed=None):
    """(q, g) [N, D] int64, to be used with normalize=False so that S = q . g^T is exact.
    "ties": D = 32, entries in {-1, 0, 1}, 35 % of the gallery entries copied from the query, one duplicated case.
    "constant": all rows equal -- every similarity tied, rho_i = i.
    "perfect": g = 5 q on distinct rows of equal norm -- every rank 0: one-hot rows (D = N) up to N = 1000; beyond (a one-hot
    operand of MAX_CASES rows is 256 MiB a side) the +-1 binary code of the row index in 13 of 32 columns, the rest +1."""
    rng = np.random.default_rng(N if seed is None else seed)
    if kind == "ties":
        q = rng.integers(-1, 2, (N, 32))
        g = np.where(rng.random((N, 32)) < 0.35, q, rng.integers(-1, 2, (N, 32)))
        if N > 2:
            q[N // 2] = q[0]
            g[N // 2] = g[0]
        return q.astype(np.int64), g.astype(np.int64)
    if kind == "constant":
        row = rng.integers(-1, 2, (1, 32))
        row[0, 0] = 1
        q = np.repeat(row, N, axis=0).astype(np.int64)
        return q, q.copy()
    if kind == "perfect":
        if N <= 1000:
            q = np.eye(N, dtype=np.int64)
        else:
            q = np.ones((N, 32), dtype=np.int64)
            q[:, :13] = 2 * ((np.arange(N)[:, None] >> np.arange(13)[None, :]) & 1) - 1
        return q, 5 * q
    raise ValueError(kind)


def beats(S):
    """b [N, N] bool: b[i][j] = j != i and (S[i][j] > S[i][i] or (S[i][j] == S[i][i] and j < i))."""
    S = np.asarray(S)
    N = S.shape[0]
    d = np.diagonal(S)[:, None]
    j, i = np.arange(N)[None, :], np.arange(N)[:, None]
    return (j != i) & ((S[:, :N] > d) | ((S[:, :N] == d) & (j < i)))


def pack(b):
    """bits [N, ceil(N / 32)] uint32: bit j & 31 of word j >> 5 = b[i][j], zeros past N."""
    N = b.shape[0]
    W = (N + 31) // 32
    full = np.zeros((N, 32 * W), dtype=bool)
    full[:, :N] = b
    return np.packbits(full, axis=1, bitorder="little").view("<u4").reshape(N, W)


def counts(b, m, ks):
    """(H_1 .. H_L, R, Q, M) int64 of the flags b for the multiplicities m."""
    m = np.asarray(m, dtype=np.int64)
    N = m.shape[0]
    rho = np.rint(b.astype(np.float32) @ m.astype(np.float32)).astype(np.int64)  # exact: every partial sum is at most N <= 2^13
    H = [int(np.sum(m * (rho < k))) for k in ks]
    R = int(np.sum(m * rho))
    Q = int(np.sum(m * ((1 << 32) // (rho + 1))))
    cum = np.cumsum(np.bincount(rho, weights=m, minlength=N + 1).astype(np.int64))
    M = int(np.argmax(2 * cum >= N))
    return np.array(H + [R, Q, M], dtype=np.int64)


def loss_terms(S, tau, rows=None):
    """fp64 [len(rows)]: log sum_{j<N} exp(S_ij / tau) - S_ii / tau, S (float32, [N, >= N]) widened before the division."""
    N = S.shape[0]
    rows = np.arange(N) if rows is None else np.asarray(rows)
    x = S[rows, :N].astype(np.float64) / np.float64(tau)
    mx = x.max(axis=1, keepdims=True)
    return (mx[:, 0] + np.log(np.exp(x - mx).sum(axis=1))) - S[rows, rows].astype(np.float64) / np.float64(tau)


@pytest.mark.parametrize("N,tied,r1,maxrank", [(65, 164, 0.23, 32), (257, 1728, 0.25, 237), (1000, 27897, 0.14, 902),
                                               (8192, 1.9e6, 0.045, 8107)])
def test_the_shared_inputs_have_real_ties_and_the_whole_rank_range(N, tied, r1, maxrank):
    q, g = make_inputs(N, "ties")
    S = q @ g.T
    b = beats(S)
    eq = (S == np.diagonal(S)[:, None]) & ~np.eye(N, dtype=bool)
    rho = b.sum(axis=1)
    print(f"N {N}: tied pairs {int(eq.sum())}, R@1 {float((rho == 0).mean()):.3f}, max rank {int(rho.max())}")
    if N == 8192:                                                                      # the table gives two digits here
        assert abs(int(eq.sum()) - tied) < 0.05e6 and abs(float((rho == 0).mean()) - r1) < 0.0005 and int(rho.max()) == maxrank
    else:
        assert int(eq.sum()) == tied and abs(float((rho == 0).mean()) - r1) < 0.005 and int(rho.max()) == maxrank
    assert (eq & b).any() and (eq & ~b).any()                                          # both branches of the tie rule
    assert np.array_equal(counts(b, np.ones(N, dtype=np.int64), (1,))[:2], [int((rho == 0).sum()), int(rho.sum())])
    qc, gc = make_inputs(N, "constant")
    assert np.array_equal(beats(qc @ gc.T).sum(axis=1), np.arange(N))
    qp, gp = make_inputs(N, "perfect")
    assert not beats(qp @ gp.T).any()
    bits = pack(b)
    assert bits.shape == (N, (N + 31) // 32) and int(bits[3, 0]) & 1 == int(b[3, 0]) and int(bits[0, 1] >> 1) & 1 == int(b[0, 33])


def test_perfect_inputs_beyond_one_hot_sizes_are_distinct_rows_of_equal_norm():
    q, g = make_inputs(8192, "perfect")
    rows = np.array([0, 1, 4095, 8191])
    S = q[rows] @ g.T
    assert (S[np.arange(4), rows] == 160).all() and ((S < 160).sum(axis=1) == 8191).all()


# ---- values -------------------------------------------------------------------------------------------------------------
def test_values_from_counts_on_hand_made_counts():
    from sm3hip import retrieval
    ranks = [0, 0, 2, 6, 1, 0, 12]                                                      # N = 7 (odd)
    for rho in (ranks, ranks + [3]):                                                     # and N = 8 (even)
        N = len(rho)
        b = np.zeros((N, N), dtype=bool)
        for i, r in enumerate(rho):                                                      # any r competitors
            b[i, [j for j in range(N) if j != i][:min(r, N - 1)]] = True
        rho = b.sum(axis=1)
        c = counts(b, np.ones(N, dtype=np.int64), (1, 5, 10))
        v = retrieval.values_from_counts(c, N)
        assert v.dtype == np.float64 and v.shape == (6,)
        for l, k in enumerate((1, 5, 10)):
            assert v[l] == float(np.sum(rho < k)) / N
        assert v[3] == 1.0 + float(rho.sum()) / N
        assert v[4] == float(sorted(rho)[(N - 1) // 2] + 1)                               # the lower median, 1-based
        exact = sum(Fraction(1, int(r) + 1) for r in rho) / N
        assert 0 <= exact - Fraction(v[5]) <= Fraction(1, 2 ** 32)
        assert v[5] == float(c[4]) / float(N * 2 ** 32)
    stacked = retrieval.values_from_counts(np.stack([c, c]), N)
    assert stacked.shape == (2, 6) and np.array_equal(stacked[1], v)
    assert retrieval.series_names((1, 5)) == ["R@1", "R@5", "mean_rank", "median_rank", "MRR"]
    # weighted: a case drawn three times counts three times, and its copies in the gallery do not compete with it
    b = np.array([[0, 1, 1], [0, 0, 0], [1, 0, 0]], dtype=bool)
    assert np.array_equal(counts(b, np.array([3, 0, 0]), (1, 2)), [3, 3, 0, 3 << 32, 0])
    assert np.array_equal(counts(b, np.array([1, 0, 2]), (1, 2)), [0, 2, 1 * 2 + 2 * 1, (1 << 32) // 3 + 2 * (1 << 31), 1])


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_settings_and_inputs_are_refused_before_any_device_work():
    from sm3hip import retrieval
    q, g = torch.randn(5, 16), torch.randn(5, 16)
    for kw in ({"bootstrap": -1}, {"bootstrap": 1.5}, {"bootstrap": True}, {"confidence": 0.0}, {"confidence": 1.0},
               {"seed": -1}, {"seed": 2 ** 64}, {"bootstrap": 4, "chunk": 0}, {"bootstrap": 4, "chunk": 5},
               {"ks": ()}, {"ks": tuple(range(1, 10))}, {"ks": (0,)}, {"ks": (1, retrieval.MAX_CASES + 1)}, {"ks": (1.0,)},
               {"ks": 3}, {"temperature": 0.0}, {"temperature": -0.1}, {"temperature": float("inf")}, {"temperature": float("nan")},
               {"max_s_bytes": 0}):
        with pytest.raises(ValueError):
            retrieval.retrieval_report(q, g, **kw)
    for bad in (q.double(), q[:4], q[:, :8], q[0], q.long(), "q", torch.zeros(0, 16), torch.zeros(5, 0)):
        with pytest.raises(ValueError):
            retrieval.retrieval_report(bad, g)
        with pytest.raises(ValueError):
            retrieval.retrieval_report(q, bad)
    for v in (float("nan"), float("inf")):
        bad = q.clone()
        bad[2, 3] = v
        with pytest.raises(ValueError, match="finite"):
            retrieval.retrieval_report(bad, g)
        with pytest.raises(ValueError, match="finite"):
            retrieval.cross_modal_report(q, bad)
    big = torch.zeros(retrieval.MAX_CASES + 1, 4)
    with pytest.raises(ValueError, match=f"MAX_CASES = {retrieval.MAX_CASES}"):
        retrieval.retrieval_report(big, big)
    with pytest.raises(ValueError, match="GPU"):                                         # CPU tensors: no fallback
        retrieval.retrieval_report(q, g)
    with pytest.raises(ValueError, match="SimCLRSkinV3"):
        retrieval.embed(torch.nn.Linear(2, 2), q, g)


def _fake(seed=3, B=5, shift=0.0, N=9, ks=(1, 5)):
    from sm3hip import retrieval
    rng = np.random.default_rng(1)
    L = len(ks)
    rep = {"N": N, "ks": list(ks), "series": retrieval.series_names(ks), "values": torch.from_numpy(rng.random(L + 3) + shift),
           "loss": 1.5 + shift, "positive_similarity": 0.5, "temperature": 0.1, "normalize": True,
           "ranks": torch.arange(N) + 1}
    if B:
        r = rng.random((B, L + 3)) + shift
        from sm3hip import report
        lo, hi = report.interval(r, 0.9)
        rep.update({"replicates": torch.from_numpy(r), "lo": torch.from_numpy(lo.copy()), "hi": torch.from_numpy(hi.copy()),
                    "bootstrap": B, "seed": seed, "confidence": 0.9})
    return rep


def test_compare_pairs_the_replicates_and_refuses_unpaired_reports(tmp_path):
    from sm3hip import retrieval
    a, b = _fake(), _fake(shift=0.25)
    z = retrieval.compare(a, a)
    assert not z["delta"].any() and not z["lo"].any() and not z["hi"].any() and float(z["frac_le_zero"].min()) == 1.0
    d = retrieval.compare(b, a)
    assert torch.allclose(d["delta"], torch.full((5,), 0.25, dtype=torch.float64)) and d["loss_delta"] == 0.25
    assert torch.allclose(d["lo"], d["hi"]) and float(d["frac_le_zero"].max()) == 0.0
    for other in (_fake(seed=4), _fake(B=4), _fake(N=10), _fake(ks=(1, 6))):
        with pytest.raises(ValueError):
            retrieval.compare(a, other)
    with pytest.raises(ValueError):
        retrieval.compare(a, {"values": 1})
    cross = {"directions": list(retrieval.DIRECTIONS), "derm->clinic": a, "clinic->derm": b}
    zc = retrieval.compare(cross, cross)
    assert all(not zc[d]["delta"].any() for d in retrieval.DIRECTIONS)
    retrieval.save(cross, str(tmp_path))
    import csv
    import json
    saved = json.load(open(tmp_path / "retrieval.json"))
    assert saved["derm->clinic"]["values"] == a["values"].tolist() and "replicates" not in saved["clinic->derm"]
    rows = list(csv.reader(open(tmp_path / "retrieval.csv")))
    assert rows[0] == ["direction", "series", "value", "lo", "hi"] and len(rows) == 1 + 2 * 7
    assert rows[1][:2] == ["derm->clinic", "R@1"] and float(rows[1][2]) == float(a["values"][0]) and float(rows[1][4]) == float(a["hi"][0])
    assert rows[7] == ["derm->clinic", "positive_similarity", "0.5", "", ""]
    line = retrieval.stats_line(a, "derm->clinic")
    assert line.startswith("derm->clinic R@1 ") and "median" in line and "MRR" in line and "loss 1.5000" in line and "[" in line


# ---- the library --------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_carry_both_entry_points():
    from sm3hip import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sm3_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("sm3_retrieval_beats", "sm3_retrieval_counts"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]) == 10, name
        assert hasattr(lib, name)
    assert lib.sm3_abi_version() == 9


def test_entry_points_reject_bad_arguments_before_any_launch():
    from sm3hip import _lib, retrieval
    lib = _lib.load()
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)  # host memory: never dereferenced by a kernel, every call below returns before a launch
    odd = C.c_void_p(p.value + 4)
    ks3 = (C.c_int32 * 3)(1, 5, 10)

    def cnt(bits=p, N=5, ks=ks3, L=3, out=p, seed=0, r0=0, c=1, point=0):
        return lib.sm3_retrieval_counts(bits, N, ks, L, out, seed, r0, c, point, None)
    for name in ("bits", "ks", "out"):
        assert cnt(**{name: None}) == -1, name
    assert cnt(N=0) == -1 and cnt(N=-3) == -1 and cnt(N=retrieval.MAX_CASES + 1) == -1
    assert cnt(c=0) == -1 and cnt(c=-1) == -1 and cnt(L=0) == -1 and cnt(L=9) == -1
    assert cnt(ks=(C.c_int32 * 3)(1, 0, 10)) == -1 and cnt(ks=(C.c_int32 * 3)(1, 5, retrieval.MAX_CASES + 1)) == -1
    assert cnt(r0=-1) == -1 and cnt(r0=2 ** 32) == -1 and cnt(r0=2 ** 32 - 1, c=2) == -1 and cnt(point=1, c=2) == -1
    assert cnt(out=odd) == -2

    def bts(S=p, ld=8, n=2, q0=0, N=5, tau=0.1, bits=p, rank=p, term=p):
        return lib.sm3_retrieval_beats(S, ld, n, q0, N, tau, bits, rank, term, None)
    for name in ("S", "bits", "rank", "term"):
        assert bts(**{name: None}) == -1, name
    assert bts(N=0) == -1 and bts(N=retrieval.MAX_CASES + 1, ld=10000) == -1 and bts(n=0) == -1 and bts(q0=-1) == -1
    assert bts(q0=4) == -1 and bts(n=6) == -1 and bts(ld=4) == -1
    assert bts(tau=0.0) == -1 and bts(tau=-1.0) == -1 and bts(tau=float("inf")) == -1 and bts(tau=float("nan")) == -1
    assert bts(term=odd) == -2


# ---- the tools ----------------------------------------------------------------------------------------------------------
def _tool(name):
    return _load("sm3_retrieval_cli_" + name, os.path.join(TOOLS, name + ".py"))


def test_the_tools_parse_their_flags():
    base = ["--data-name", "synthetic", "--data-path", "-"]
    p = _tool("backbone_retrieval").get_parser()
    d = p.parse_args(base)
    assert (d.retrieval_k, d.retrieval_t, d.bootstrap, d.bootstrap_seed, d.confidence) == ([1, 5, 10], 0.1, 0, 0, 0.95)
    assert d.save_embeddings is False and d.against is None and d.arch_version == "v3" and d.proj_dim == 128
    a = p.parse_args(base + ["--retrieval-k", "1", "3", "--retrieval-t", "0.07", "--bootstrap", "2000", "--bootstrap-seed",
                             str(2 ** 63 + 11), "--confidence", "0.9", "--save-embeddings", "--against", "o/retrieval_embeddings.pt",
                             "-a", "resnet18", "--arch-version", "v32", "--proj-dim", "64", "--amp", "--amp-dtype", "bf16"])
    assert (a.retrieval_k, a.retrieval_t, a.bootstrap, a.bootstrap_seed) == ([1, 3], 0.07, 2000, 2 ** 63 + 11)
    assert a.against == "o/retrieval_embeddings.pt" and a.save_embeddings and a.arch_version == "v32" and a.proj_dim == 64
    t = _tool("backbone_train").get_parser().parse_args(base)
    assert (t.retrieval_freq, t.retrieval_cases) == (0, 256)
    b = _tool("retrieval_bench").get_parser().parse_args([])
    assert b.bootstrap == 2000


def test_backbone_retrieval_refuses_before_the_device_is_touched(tmp_path, monkeypatch):
    br = _tool("backbone_retrieval")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("the device was touched")))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: (_ for _ in ()).throw(AssertionError("the device was touched")))
    syn = ["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "--log-path", str(tmp_path)]
    for extra in (["--retrieval-k", "0"], ["--retrieval-k"] + [str(k) for k in range(1, 10)], ["--retrieval-k", "8193"],
                  ["--retrieval-t", "0"], ["--bootstrap", "-1"], ["--confidence", "1.0"], ["--bootstrap-seed", str(2 ** 64)],
                  ["-b", "8", "--val-steps", "1025"],                                    # N = 8200 > MAX_CASES
                  ["--against", str(tmp_path / "missing.pt")]):
        with pytest.raises(SystemExit) as e:
            br.main(syn + extra)
        assert e.value.code not in (0, None), extra
    with pytest.raises(SystemExit):
        br.main(["--data-name", "synthetic", "--data-path", "-", "-a", "vgg16", "--log-path", str(tmp_path)])
    import shutil
    meta = os.path.join(ROOT, "tests", "golden", "derm7pt_meta")                         # a derm7pt tree without its images
    tree = tmp_path / "7PC"
    os.makedirs(tree / "images")
    for f in ("meta.csv", "train_indexes.csv", "valid_indexes.csv", "test_indexes.csv"):
        shutil.copy(os.path.join(meta, f), tree / f)
    real = ["--data-name", "SevenPCBaseDataset", "--data-path", str(tree), "-a", "resnet18", "--log-path", str(tmp_path)]
    for extra in ([], ["--pretrain-path", str(tmp_path / "none.pth")]):                  # real data needs a checkpoint
        with pytest.raises(SystemExit, match="checkpoint"):
            br.main(real + extra)
    with pytest.raises(SystemExit, match="checkpoint"):
        br.main(syn + ["--pretrain-path", str(tmp_path / "none.pth")])
    bt = _tool("backbone_train")
    args = bt.get_parser().parse_args(["--data-name", "synthetic", "--data-path", "-", "--retrieval-freq", "1", "--retrieval-cases", "0"])
    with pytest.raises(SystemExit, match="retrieval"):
        bt.main(0, args)
