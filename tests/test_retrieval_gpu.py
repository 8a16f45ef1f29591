"""GPU: the cross-modal retrieval report (csrc/retrieval.hip, sm3hip/retrieval.py, tools/backbone_retrieval.py and
tools/backbone_train.py --retrieval-freq).

  * G1 sm3_retrieval_beats on integer-valued embeddings (S exact, ties real): S == the integer matmul, bits and rank == the
    restatement of tests/test_retrieval_cpu.py, padding bits 0, every output element overwritten, the loss terms within
    4 N 2^-53 (1 + |term|) of the fp64 restatement on the device's own S, a row-chunked run == the one-call run;
  * G2 sm3_retrieval_counts == the integer restatement with the multiplicities of tests/test_report_cpu.py: the point record and
    replicates, seeds that use both key words, replicate offsets up to 2^20, L = 3 and L = 8, any cut of a replicate range, a
    replicate with a case drawn four times or more (more than two bit-planes);
  * G3 the wrappers refuse what the kernels do not take;
  * G4 the report: equal bits whatever chunk, max_s_bytes or bootstrap size; replicates == the restatement through the
    library; compare(a, a) zero; symmetric input, equal directions; continuous embeddings against a torch fp64 argsort;
  * G5 embed: against the fp64 eval-mode projectors on the engine's features (T0 bound 1e-4), batches of 1, 2 and 6 give each
    case the same bits, the state_dict untouched; bf16: the batch independence;
  * G6 the tools."""
import csv
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
DEV = "cuda:0"
SENTINEL = -0x0123456789ABCDEF
NS = [1, 2, 5, 31, 32, 33, 63, 64, 65, 255, 257, 1000, "MAX_CASES"]
RUNS = ((7, 0, 1), (2 ** 32 + 5, 1000, 3), (2 ** 63 + 11, 2 ** 20 - 3, 70))


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REF = _load("sm3_retrieval_ref", os.path.join(ROOT, "tests", "test_retrieval_cpu.py"))  # make_inputs, beats, pack, counts, ...


def _tool(name):
    return _load("sm3_retrieval_gpu_" + name, os.path.join(TOOLS, name + ".py"))


def _n(N):
    from sm3hip import retrieval
    return retrieval.MAX_CASES if N == "MAX_CASES" else N


@functools.lru_cache(maxsize=3)
def _case(N, kind):
    """(q, g int64, S int32 = q . g^T, b bool, bits uint32) of the shared inputs, computed once."""
    q, g = REF.make_inputs(N, kind)
    S = np.rint(q.astype(np.float64) @ g.astype(np.float64).T).astype(np.int32)      # exact: |entries| small
    b = REF.beats(S)
    return q, g, S, b, REF.pack(b)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.numpy().view(np.uint64), b.numpy().view(np.uint64))


# ---- G1 -----------------------------------------------------------------------------------------------------------------
def _device_beats(q, g, tau, max_s_bytes=1 << 30, want_s=False):
    """retrieval.beats with sentinel-filled outputs, and the device's own S of the one-call run."""
    from sm3hip import ops, retrieval
    from sm3hip.knn import KNNBank
    N = q.shape[0]
    dq, dg = (torch.from_numpy(a).float().to(DEV) for a in (q, g))
    bits, rank, term, diag = retrieval.beats(dq, dg, tau, max_s_bytes)
    torch.cuda.synchronize()
    S = None
    if want_s:
        bank = KNNBank(dg, torch.zeros(N, dtype=torch.int32, device=DEV), 1)
        S = torch.empty(N, bank.ld, dtype=torch.float32, device=DEV)
        qp = dq if bank.Dp == dq.shape[1] else torch.nn.functional.pad(dq, (0, bank.Dp - dq.shape[1]))
        bank.similarity(qp.contiguous(), S)
        W = (N + 31) // 32
        sb = torch.full((N, W), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        sr = torch.full((N,), -77, dtype=torch.int32, device=DEV)
        st = torch.full((N,), float("nan"), dtype=torch.float64, device=DEV)
        ops.retrieval_beats(S, 0, N, tau, sb, sr, st)                                 # every output element is overwritten
        torch.cuda.synchronize()
        assert torch.equal(sb, bits) and torch.equal(sr, rank) and not bool(torch.isnan(st).any())
        assert np.array_equal(st.cpu().numpy().view(np.uint64), term.cpu().numpy().view(np.uint64))
        S = S.cpu().numpy()
    return bits.cpu().numpy().view(np.uint32), rank.cpu().numpy(), term.cpu().numpy(), diag.cpu().numpy(), S


@pytest.mark.parametrize("N", NS)
def test_beats_equal_the_restatement(N):
    big = N == "MAX_CASES"
    N = _n(N)
    tau = 0.5
    for kind in ("ties", "constant", "perfect"):
        q, g, S, b, want_bits = _case(N, kind)
        bits, rank, term, diag, dS = _device_beats(q, g, tau, want_s=True)
        assert dS.shape[1] >= N and dS.shape[1] % 4 == 0 and np.array_equal(dS[:, :N], S), kind
        assert not dS[:, N:].any()                                                      # the padding columns of S
        assert bits.shape == (N, (N + 31) // 32) and np.array_equal(bits, want_bits), kind
        if N % 32:
            assert not (bits[:, -1] >> np.uint32(N % 32)).any()                        # padding bits are 0
        assert np.array_equal(rank, b.sum(axis=1)), kind
        assert np.array_equal(diag.astype(np.int64), np.diagonal(S))
        if kind == "constant":
            assert np.array_equal(rank, np.arange(N))
        if kind == "perfect":
            assert not rank.any()
        rows = np.arange(N)
        want = np.concatenate([REF.loss_terms(dS, tau, rows[a:a + 1024]) for a in range(0, N, 1024)])  # row blocks: memory
        err = np.abs(term[rows] - want)
        bound = 4 * N * 2.0 ** -53 * (1 + np.abs(want))
        print(f"N {N} {kind}: max loss-term error {err.max():.3e}, bound {bound.min():.3e}")
        assert (err <= bound).all(), kind
        # row chunks (q0 > 0, n < N) give the same bits as the one call
        if N > 1:
            ld = dS.shape[1]
            for rows_per in ((1, 3) if N <= 65 else (max(1, N // 3),)):
                b2, r2, t2, d2, _ = _device_beats(q, g, tau, max_s_bytes=4 * ld * rows_per)
                assert np.array_equal(b2, bits) and np.array_equal(r2, rank) and np.array_equal(d2, diag), (kind, rows_per)
                assert np.array_equal(t2.view(np.uint64), term.view(np.uint64)), (kind, rows_per)


# ---- G2 -----------------------------------------------------------------------------------------------------------------
def _device_counts(bits, ks, seed, r0, c, point=False):
    from sm3hip import ops
    out = torch.full((c, len(ks) + 3), SENTINEL, dtype=torch.int64, device=DEV)
    ops.retrieval_counts(bits, ks, out, seed, r0, point=point)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not (got == SENTINEL).any()                                                # every element is overwritten
    return got


@pytest.mark.parametrize("N", NS)
def test_counts_equal_the_integer_restatement(N):
    from sm3hip import retrieval
    big = N == "MAX_CASES"
    N = _n(N)
    k8 = (1, 2, 3, 5, 10, 100, N, retrieval.MAX_CASES)
    for kind, run, ks in zip(("ties", "constant", "ties"), RUNS, ((1, 5, 10), k8, k8)):
        seed, r0, c = run
        c = 3 if big else c                                                           # the host restatement is the slow side
        b, host_bits = _case(N, kind)[3:]
        bits = torch.from_numpy(host_bits.view(np.int32)).to(DEV)
        point = _device_counts(bits, ks, seed, 0, 1, point=True)
        assert np.array_equal(point[0], REF.counts(b, np.ones(N, dtype=np.int64), ks)), (kind, "point")
        got = _device_counts(bits, ks, seed, r0, c)
        for j in range(c):                                                            # every replicate of the call
            want = REF.counts(b, REF.multiplicities(seed, r0 + j, N), ks)
            assert np.array_equal(got[j], want), (kind, seed, r0 + j)
        if not big:                                                                   # any cut of [r0, r0 + c) is the one call
            parts = [_device_counts(bits, ks, seed, r0 + k, min(8, c - k)) for k in range(0, c, 8)]
            assert np.array_equal(np.concatenate(parts), got)
            for s2, r2, c2 in RUNS:                                                   # every seed, offset and count on this input
                g2 = _device_counts(bits, ks, s2, r2, c2)
                assert np.array_equal(g2[c2 - 1], REF.counts(b, REF.multiplicities(s2, r2 + c2 - 1, N), ks)), (kind, s2, r2)
    if N >= 4:  # a replicate in which a case is drawn four times or more: three bit-planes at the least
        b, host_bits = _case(N, "ties")[3:]
        bits = torch.from_numpy(host_bits.view(np.int32)).to(DEV)
        r = next(r for r in range(100000) if REF.multiplicities(7, r, N).max() >= 4)
        m = REF.multiplicities(7, r, N)
        print(f"N {N}: replicate {r} draws a case {int(m.max())} times")
        assert np.array_equal(_device_counts(bits, (1, 5, 10), 7, r, 1)[0], REF.counts(b, m, (1, 5, 10)))


def test_counts_ignore_whatever_the_padding_bits_hold():
    N = 45
    b, host_bits = _case(N, "ties")[3:]
    dirty = host_bits.copy()
    dirty[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(N % 32)
    got = _device_counts(torch.from_numpy(dirty.view(np.int32)).to(DEV), (1, 5, 10), 7, 0, 4)
    for j in range(4):
        assert np.array_equal(got[j], REF.counts(b, REF.multiplicities(7, j, N), (1, 5, 10)))


# ---- G3 -----------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_what_the_kernels_do_not_take():
    from sm3hip import ops
    N = 5
    bits = torch.zeros(N, 1, dtype=torch.int32, device=DEV)
    out = torch.zeros(2, 6, dtype=torch.int64, device=DEV)
    ks = (1, 5, 10)
    with pytest.raises(ValueError):
        ops.retrieval_counts(bits, ks, out, 0, 0, point=True)                         # the point estimate is one record
    with pytest.raises(ValueError):
        ops.retrieval_counts(bits, ks, out, 2 ** 64, 0)
    with pytest.raises(ValueError):
        ops.retrieval_counts(bits.long(), ks, out, 0, 0)
    with pytest.raises(ValueError):
        ops.retrieval_counts(bits, ks, out[:, :5], 0, 0)
    with pytest.raises(ValueError):
        ops.retrieval_counts(bits, ks, out.int(), 0, 0)
    with pytest.raises(ValueError):
        ops.retrieval_counts(bits.cpu(), ks, out, 0, 0)
    with pytest.raises(ValueError):
        ops.retrieval_counts(torch.zeros(N, 2, dtype=torch.int32, device=DEV), ks, out, 0, 0)
    for bad in ((), (0, 1, 2), (1, 5, 8193), (1.0, 5, 10), tuple(range(1, 10))):
        with pytest.raises(ValueError):
            ops.retrieval_counts(bits, bad, out, 0, 0)
    S = torch.zeros(3, 8, dtype=torch.float32, device=DEV)
    rank = torch.zeros(3, dtype=torch.int32, device=DEV)
    term = torch.zeros(3, dtype=torch.float64, device=DEV)
    b3 = torch.zeros(3, 1, dtype=torch.int32, device=DEV)
    ops.retrieval_beats(S, 2, N, 0.1, b3, rank, term)                                  # rows 2 .. 4 of 5: the last that fit
    for kw in (dict(q0=3), dict(q0=-1), dict(N=9), dict(N=0), dict(temperature=0.0), dict(temperature=float("inf")),
               dict(S=S.double()), dict(S=S.cpu()), dict(S=S[:, :7]), dict(bits=torch.zeros(3, 2, dtype=torch.int32, device=DEV)),
               dict(rank=rank.long()), dict(term=term.float()), dict(term=term[:2]), dict(rank=rank[:2])):
        a = dict(S=S, q0=2, N=N, temperature=0.1, bits=b3, rank=rank, term=term)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.retrieval_beats(**a)
    torch.cuda.synchronize()


# ---- G4 -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair395():
    q, g = REF.make_inputs(395, "ties", 42)
    return torch.from_numpy(q).float().to(DEV), torch.from_numpy(g).float().to(DEV)


def test_the_report_does_not_depend_on_chunk_s_bytes_or_bootstrap_size(pair395):
    from sm3hip import report, retrieval
    q, g = pair395
    before = q.clone(), g.clone()
    B, seed = 64, 2 ** 63 + 11
    kw = dict(normalize=False, temperature=0.5, seed=seed)
    first = retrieval.retrieval_report(q, g, bootstrap=B, **kw)
    assert first["replicates"].shape == (B, 6) and first["values"].shape == (6,) and first["ranks"].shape == (395,)
    assert first["ranks"].dtype == torch.int64 and int(first["ranks"].min()) >= 1 and first["N"] == 395
    assert first["series"] == ["R@1", "R@5", "R@10", "mean_rank", "median_rank", "MRR"]
    for extra in (dict(chunk=1), dict(chunk=7), dict(chunk=B), dict(max_s_bytes=4 * 396 * 10), dict(max_s_bytes=1, chunk=5)):
        again = retrieval.retrieval_report(q, g, bootstrap=B, **kw, **extra)
        for key in ("values", "replicates", "lo", "hi"):
            assert _same(first[key], again[key]), (extra, key)
        assert torch.equal(first["ranks"], again["ranks"]) and torch.equal(first["counts"], again["counts"])
        assert again["loss"] == first["loss"] and again["positive_similarity"] == first["positive_similarity"]
    longer = retrieval.retrieval_report(q, g, bootstrap=100, **kw)
    assert _same(longer["replicates"][:B].contiguous(), first["replicates"]) and _same(longer["values"], first["values"])
    other = retrieval.retrieval_report(q, g, bootstrap=B, normalize=False, temperature=0.5, seed=seed + 1)
    assert not _same(other["replicates"], first["replicates"]) and _same(other["values"], first["values"])
    none = retrieval.retrieval_report(q, g, normalize=False, temperature=0.5)
    assert "replicates" not in none and _same(none["values"], first["values"])
    lo, hi = report.interval(first["replicates"].numpy(), 0.95)
    assert np.array_equal(first["lo"].numpy(), lo) and np.array_equal(first["hi"].numpy(), hi)
    assert bool((first["lo"] <= first["hi"]).all())
    assert torch.equal(q, before[0]) and torch.equal(g, before[1])                      # inputs are not modified


def test_replicates_are_the_restatement_through_the_library(pair395):
    from sm3hip import retrieval
    q, g = pair395
    N = 395
    rep = retrieval.retrieval_report(q, g, ks=(1, 5, 10), normalize=False, temperature=0.5, bootstrap=64, seed=7)
    S = np.rint(q.cpu().numpy().astype(np.float64) @ g.cpu().numpy().astype(np.float64).T).astype(np.int64)
    b = REF.beats(S)
    point = REF.counts(b, np.ones(N, dtype=np.int64), (1, 5, 10))
    assert np.array_equal(rep["counts"].numpy(), point)
    assert np.array_equal(rep["values"].numpy().view(np.uint64), retrieval.values_from_counts(point, N).view(np.uint64))
    assert np.array_equal(rep["ranks"].numpy(), b.sum(axis=1) + 1)
    for r in range(64):
        want = retrieval.values_from_counts(REF.counts(b, REF.multiplicities(7, r, N), (1, 5, 10)), N)
        assert np.array_equal(rep["replicates"][r].numpy().view(np.uint64), want.view(np.uint64)), r
    terms = REF.loss_terms(S.astype(np.float32), 0.5)
    seq = 0.0
    for t in terms:
        seq = seq + float(t)
    assert abs(rep["loss"] - seq / N) <= 4 * N * 2.0 ** -53 * (1 + abs(seq / N))
    dsum = 0.0
    for v in np.diagonal(S):
        dsum = dsum + float(v)
    assert rep["positive_similarity"] == dsum / N


def test_compare_with_itself_is_zero_and_a_symmetric_input_has_equal_directions(pair395):
    from sm3hip import retrieval
    q, g = pair395
    kw = dict(normalize=False, temperature=0.5, bootstrap=64, seed=3)
    a = retrieval.cross_modal_report(q, g, **kw)
    assert a["directions"] == ["derm->clinic", "clinic->derm"]
    assert not _same(a["derm->clinic"]["replicates"], a["clinic->derm"]["replicates"])
    z = retrieval.compare(a, a)
    for d in a["directions"]:
        for key in ("delta", "lo", "hi"):
            assert not z[d][key].any(), (d, key)
        assert float(z[d]["frac_le_zero"].min()) == 1.0 and z[d]["loss_delta"] == 0.0
    one = retrieval.compare(a["derm->clinic"], a["clinic->derm"])                     # paired: one seed, the same cases
    assert one["delta"].any() and bool((one["lo"] <= one["hi"]).all())
    with pytest.raises(ValueError, match="seed"):
        retrieval.compare(a["derm->clinic"], retrieval.retrieval_report(q, g, normalize=False, temperature=0.5, bootstrap=64, seed=4))
    s = retrieval.cross_modal_report(q, q, **kw)                                        # q is g: S is symmetric
    for key in ("values", "replicates", "lo", "hi"):
        assert _same(s["derm->clinic"][key], s["clinic->derm"][key]), key
    assert torch.equal(s["derm->clinic"]["ranks"], s["clinic->derm"]["ranks"]) and s["derm->clinic"]["loss"] == s["clinic->derm"]["loss"]


def test_continuous_embeddings_against_a_torch_argsort():
    from sm3hip import retrieval
    from sm3hip.knn import KNNBank, normalize
    gen = torch.Generator(device=DEV).manual_seed(11)
    N, D = 395, 128
    base = torch.randn(N, D, device=DEV, generator=gen)
    q = base + 1.5 * torch.randn(N, D, device=DEV, generator=gen)
    g = base + 1.5 * torch.randn(N, D, device=DEV, generator=gen)
    rep = retrieval.retrieval_report(q, g, ks=(1, 5, 10), temperature=0.1)
    qn, gn = normalize(q), normalize(g)
    bank = KNNBank(gn, torch.zeros(N, dtype=torch.int32, device=DEV), 1)
    S = torch.empty(N, bank.ld, dtype=torch.float32, device=DEV)
    bank.similarity(qn, S)
    order = torch.argsort(S[:, :N].double(), dim=1, descending=True, stable=True)      # equal similarities: lower index first
    rank = (order == torch.arange(N, device=DEV)[:, None]).double().argmax(dim=1).cpu().numpy() + 1
    assert np.array_equal(rep["ranks"].numpy(), rank)
    v = rep["values"].numpy()
    assert 0.02 < v[0] < 0.98                                                           # neither trivial
    for l, k in enumerate((1, 5, 10)):
        assert v[l] == float((rank <= k).sum()) / N
    assert v[3] == 1.0 + float((rank - 1).sum()) / N and v[4] == float(np.sort(rank)[(N - 1) // 2])
    assert abs(v[5] - float(np.mean(1.0 / rank))) <= 2.0 ** -32
    x = S[:, :N].double() / 0.1
    want = float((torch.logsumexp(x, dim=1) - x.diagonal()).mean())
    assert abs(rep["loss"] - want) <= 8 * N * 2.0 ** -53 * (1 + abs(want))               # N additions on either side
    assert abs(rep["positive_similarity"] - float(S[:, :N].diagonal().double().mean())) <= 2 * N * 2.0 ** -53


# ---- G5 -----------------------------------------------------------------------------------------------------------------
def _model(cls_name, dtype):
    from src.models import simclr
    torch.manual_seed(5)
    model = getattr(simclr, cls_name)("resnet18", None, 128, 0.1)
    model.sm3_dtype = dtype
    gen = torch.Generator().manual_seed(6)
    projs = list(model.cross_proj) if cls_name == "SimCLRSkinV32" else [model.cross_proj]
    for p in projs:                                                                     # non-trivial running statistics
        for m in p:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(0.3 * torch.randn(m.running_mean.shape, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))
                m.num_batches_tracked.fill_(17)
    return model.to(DEV).eval(), projs


@pytest.mark.parametrize("cls_name", ["SimCLRSkinV32", "SimCLRSkinV3"])
def test_embed_is_the_eval_mode_projection_and_does_not_depend_on_the_batch(cls_name):
    from sm3hip import retrieval
    model, projs = _model(cls_name, torch.float32)
    gen = torch.Generator(device=DEV).manual_seed(7)
    derm, clinic = torch.randn(6, 3, 64, 64, device=DEV, generator=gen), torch.randn(6, 3, 64, 64, device=DEV, generator=gen)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    zd, zc = retrieval.embed(model, derm, clinic)
    assert zd.shape == zc.shape == (6, 128) and zd.dtype == torch.float32 and zd.is_cuda
    feats = model.extract(derm, clinic)                                                 # eval mode: the engine's features
    for z, f, p in zip((zd, zc), feats, (projs[0], projs[-1])):
        p64 = __import__("copy").deepcopy(p).double().eval()
        with torch.no_grad():
            z64 = p64(f.double())
        err, scale = float((z.double() - z64).abs().max()), float(z64.abs().max())
        print(f"{cls_name}: max |z - z64| {err:.3e}, max |z64| {scale:.3e}, ratio {err / scale:.3e}")
        assert err <= 1e-4 * scale
    for n in (1, 2):
        for i in range(0, 6, n):
            a, b = retrieval.embed(model, derm[i:i + n], clinic[i:i + n])
            assert torch.equal(a, zd[i:i + n]) and torch.equal(b, zc[i:i + n]), (n, i)
    model.train()                                                                       # the modules' flags do not matter
    a, b = retrieval.embed(model, derm, clinic)
    assert torch.equal(a, zd) and torch.equal(b, zc) and model.training
    after = model.state_dict()
    assert sorted(after) == sorted(before) and all(torch.equal(after[k], before[k]) for k in before)


def test_embed_in_bf16_does_not_depend_on_the_batch():
    from sm3hip import retrieval
    model, _ = _model("SimCLRSkinV32", torch.bfloat16)
    gen = torch.Generator(device=DEV).manual_seed(8)
    derm, clinic = torch.randn(6, 3, 64, 64, device=DEV, generator=gen), torch.randn(6, 3, 64, 64, device=DEV, generator=gen)
    zd, zc = retrieval.embed(model, derm, clinic)
    assert bool(torch.isfinite(zd).all()) and bool(torch.isfinite(zc).all())
    for n in (1, 2):
        for i in range(0, 6, n):
            a, b = retrieval.embed(model, derm[i:i + n], clinic[i:i + n])
            assert torch.equal(a, zd[i:i + n]) and torch.equal(b, zc[i:i + n]), (n, i)


# ---- G6 -----------------------------------------------------------------------------------------------------------------
def _flat(obj, prefix=""):
    """Every tensor of a nested checkpoint entry, by path."""
    if isinstance(obj, torch.Tensor):
        return {prefix: obj}
    out = {}
    if isinstance(obj, dict):
        for k, v in obj.items():
            out.update(_flat(v, f"{prefix}/{k}"))
    elif isinstance(obj, (list, tuple)):
        for k, v in enumerate(obj):
            out.update(_flat(v, f"{prefix}/{k}"))
    return out


TRAIN = ["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "--arch-version", "v32", "--synthetic-kind", "latent",
         "-b", "4", "--img-sz", "64", "64", "--epochs", "2", "--steps-per-epoch", "2", "--temperature", "0.1"]


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """backbone_train without and with --retrieval-freq 1: (log path of the run with the flag, both histories, its output)."""
    import contextlib
    import io
    bt = _tool("backbone_train")
    root = tmp_path_factory.mktemp("retrieval_train")
    hist, outs = [], []
    for name, extra in (("plain", []), ("flag", ["--retrieval-freq", "1", "--retrieval-cases", "8"])):
        args = bt.get_parser().parse_args(TRAIN + ["--log-path", str(root / name)] + extra)
        args.world_size = 1
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            hist.append(bt.main(0, args))
        outs.append(buf.getvalue())
    return root, hist, outs


def test_training_does_not_notice_the_retrieval_flag(trained):
    root, hist, outs = trained
    assert outs[0].count("Retrieval epoch") == 0 and outs[1].count("Retrieval epoch") == 2
    lines = [l for l in outs[1].splitlines() if l.startswith("Retrieval epoch")]
    assert lines[0].startswith("Retrieval epoch: [0] derm->clinic R@1 ") and "| clinic->derm R@1 " in lines[0]
    assert " R@5 " in lines[1] and " median " in lines[1] and "| loss " in lines[1]
    assert hist[0] == hist[1] and len(hist[0]) == 2
    a = torch.load(root / "plain" / "checkpoint.pth.tar", map_location="cpu", weights_only=False)
    b = torch.load(root / "flag" / "checkpoint.pth.tar", map_location="cpu", weights_only=False)
    assert a["epoch"] == b["epoch"] == 2
    for key in ("state_dict", "optimizer", "scaler"):
        fa, fb = _flat(a[key]), _flat(b[key])
        assert sorted(fa) == sorted(fb) and (key == "scaler" or len(fa) > 0), key
        for k in fa:
            assert fa[k].dtype == fb[k].dtype and torch.equal(fa[k], fb[k]), (key, k)


def _check_files(log, rep):
    """retrieval.json and retrieval.csv of a tool run agree with each other and with the report `rep`."""
    saved = json.load(open(os.path.join(log, "retrieval.json")))
    rows = list(csv.reader(open(os.path.join(log, "retrieval.csv"))))
    assert rows[0] == ["direction", "series", "value", "lo", "hi"]
    by = {(r[0], r[1]): r[2:] for r in rows[1:]}
    for d in ("derm->clinic", "clinic->derm"):
        s, r = saved[d], rep[d]
        assert s["values"] == r["values"].tolist() and s["series"] == r["series"] and s["N"] == r["N"]
        assert s["loss"] == r["loss"] and s["positive_similarity"] == r["positive_similarity"] and "replicates" not in s
        assert by[(d, "loss")] == [repr(r["loss"]), "", ""]
        for i, name in enumerate(s["series"]):
            assert float(by[(d, name)][0]) == s["values"][i]
            if "lo" in r:
                assert s["lo"] == r["lo"].tolist() and s["hi"] == r["hi"].tolist() and s["bootstrap"] == r["bootstrap"]
                assert [float(v) for v in by[(d, name)][1:]] == [s["lo"][i], s["hi"][i]]


def test_backbone_retrieval_on_the_trained_checkpoint(trained, tmp_path, capsys):
    from sm3hip import retrieval
    root = trained[0]
    br = _tool("backbone_retrieval")
    base = ["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "--arch-version", "v32", "-b", "4", "--img-sz", "64",
            "64", "--val-steps", "3", "--pretrain-path", str(root / "flag" / "checkpoint.pth.tar"), "--bootstrap", "16",
            "--bootstrap-seed", "5", "--retrieval-k", "1", "3"]
    out = br.main(base + ["--save-embeddings", "--log-path", str(tmp_path / "a")])
    text = capsys.readouterr().out
    assert "loaded pre-trained" in text and text.count("retrieval N=12: derm->clinic R@1") == 1
    assert text.count("retrieval N=12: clinic->derm R@1") == 1
    emb = torch.load(tmp_path / "a" / "retrieval_embeddings.pt", map_location="cpu", weights_only=False)
    assert emb["derm"].shape == emb["clinic"].shape == (12, 128) and torch.equal(emb["derm"], out["derm"].cpu())
    rep = retrieval.cross_modal_report(emb["derm"].to(DEV), emb["clinic"].to(DEV), ks=(1, 3), bootstrap=16, seed=5)
    for d in rep["directions"]:                                                          # the saved embeddings reproduce the run
        for key in ("values", "replicates", "lo", "hi"):
            assert _same(rep[d][key], out["report"][d][key]), (d, key)
    _check_files(str(tmp_path / "a"), rep)
    again = br.main(base + ["--log-path", str(tmp_path / "b"), "--against", str(tmp_path / "a" / "retrieval_embeddings.pt")])
    text = capsys.readouterr().out
    assert torch.equal(again["derm"].cpu(), emb["derm"]) and torch.equal(again["clinic"].cpu(), emb["clinic"])
    assert text.count("retrieval difference to") == 2
    cmp = json.load(open(tmp_path / "b" / "retrieval_compare.json"))
    for d in rep["directions"]:                                                          # --against on itself: zero differences
        assert not any(cmp[d]["delta"]) and not any(cmp[d]["lo"]) and not any(cmp[d]["hi"]) and cmp[d]["loss_delta"] == 0.0
        assert not again["compare"][d]["delta"].any()
    assert not os.path.exists(tmp_path / "b" / "retrieval_embeddings.pt")


def test_backbone_retrieval_on_a_derm7pt_tree(trained, tmp_path, capsys):
    from sm3hip import retrieval
    from src.utils.data.datasets import read_split
    KNN = _load("sm3_retrieval_knn_helpers", os.path.join(ROOT, "tests", "test_knn_gpu.py"))  # _write_tree
    tree = KNN._write_tree(tmp_path / "7PC")
    br = _tool("backbone_retrieval")
    out = br.main(["--data-name", "SevenPCBaseDataset", "--data-path", str(tree), "-j", "4", "--mean", "0.7833", "0.6712", "0.6026",
                   "--std", "0.2139", "0.2472", "0.2571", "-a", "resnet18", "--arch-version", "v32", "-b", "6", "--img-sz", "64",
                   "64", "--pretrain-path", str(trained[0] / "flag" / "checkpoint.pth.tar"), "--bootstrap", "8",
                   "--log-path", str(tmp_path / "out")])
    N = len(read_split(str(tree), "test")[2])
    assert out["derm"].shape == (N, 128) and out["report"]["derm->clinic"]["N"] == N
    assert f"retrieval N={N}: derm->clinic" in capsys.readouterr().out
    _check_files(str(tmp_path / "out"), out["report"])
    rep = retrieval.cross_modal_report(out["derm"], out["clinic"], bootstrap=8)
    assert _same(rep["clinic->derm"]["replicates"], out["report"]["clinic->derm"]["replicates"])
