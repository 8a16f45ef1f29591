"""GPU: the weighted kNN evaluator (sm3_knn_vote, sm3hip/knn.py, KNNOnlineEvaluator, tools/backbone_knn.py) against the
reference's own predictions (golden) and an fp64 torch restatement of the reference's predict: sort -> gather -> exp(s / T)
-> scatter-sum.  The restatement takes S from the same gather-GEMM the product path uses (checked against fp64 separately),
so neighbour selection and vote sums are compared on identical similarities."""
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
DERM7PT_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]


def _restate(S, n_valid, targets, classes, k, T):
    """fp64 votes of the reference's predict on S[:, :n_valid] (ties: lower index first) and the neighbours."""
    S = S[:, :n_valid].double()
    val, idx = torch.sort(S, dim=1, descending=True, stable=True)
    val, idx = val[:, :k], idx[:, :k]
    w = torch.exp(val / float(np.float32(T)))
    t = targets.reshape(n_valid, -1).long()
    votes = [torch.zeros(S.shape[0], c, dtype=torch.float64, device=S.device).scatter_add_(1, t[idx, l], w)
             for l, c in enumerate(classes)]
    return votes, idx, val


def _features(g, n, d):
    x = torch.randn(n, d, generator=g, device=DEV)
    return x / x.norm(dim=1, keepdim=True)


def _labels(g, n, classes):
    return torch.stack([torch.randint(0, c, (n,), generator=g, device=DEV) for c in classes], dim=1)


def test_predict_equals_the_reference_on_every_golden_case(golden_dir):
    from src.models.evaluator import KNNOnlineEvaluator
    g = np.load(os.path.join(golden_dir, "knn_ref.npz"))
    for name in g["cases"]:
        k, C = [int(v) for v in g[f"{name}_meta"]]
        ev = KNNOnlineEvaluator(None, None, C, k=k, temperature=float(g[f"{name}_temperature"]))
        q, bank = torch.from_numpy(g[f"{name}_query"]).to(DEV), torch.from_numpy(g[f"{name}_bank"]).to(DEV)
        t = torch.from_numpy(g[f"{name}_targets"]).to(DEV)
        pred = ev.predict(q, bank, t)
        assert torch.equal(pred.cpu(), torch.from_numpy(g[f"{name}_pred_labels"])), name


# (B, N, D, k, labels, bank block bytes): N up to 2^18, k in {1, 7, 200, 1024}, D in {128, 1000 (padded), 4096}; the last
# two also multiply the bank in column blocks (4 GiB bank; a small block size over a bank whose N is not a multiple of 4)
SHAPES = [(64, 2 ** 18, 128, 200, 8, None), (32, 2 ** 18, 128, 1024, 1, None), (16, 5000, 1000, 7, 8, None),
          (8, 3000, 4096, 1, 1, None), (8, 2 ** 18, 4096, 1024, 8, None), (8, 1001, 96, 200, 8, 1 << 16)]


@pytest.mark.parametrize("B,N,D,k,L,block", SHAPES)
def test_scores_against_the_fp64_restatement(B, N, D, k, L, block):
    from sm3hip.knn import KNNBank, knn_scores
    g = torch.Generator(device=DEV).manual_seed(N + D + k)
    classes = DERM7PT_CLASSES if L == 8 else [5]
    bank_f, q = _features(g, N, D), _features(g, B, D)
    targets = _labels(g, N, classes)
    bank = KNNBank(bank_f, targets, classes) if block is None else KNNBank(bank_f, targets, classes, block_bytes=block)
    if block is not None:
        assert bank.blocks > 1 and bank.ld > N
    if D == 4096 and N == 2 ** 18:
        assert bank.blocks == 2
    T = 0.07
    votes, (idx, sim) = knn_scores(q, bank, k=k, temperature=T, neighbors=True)
    # the similarities the product path votes on: the same GEMM, checked against fp64
    qp = torch.nn.functional.pad(q, (0, bank.Dp - D))
    S = torch.empty(B, bank.ld, device=DEV)
    bank.similarity(qp, S)
    S64 = q.double() @ bank_f.double().T
    assert float((S[:, :N].double() - S64).abs().max()) < 1e-5
    want, widx, wval = _restate(S, N, targets, classes, k, T)
    assert torch.equal(idx.long(), widx) and torch.equal(sim.double(), wval)
    for l in range(L):
        torch.testing.assert_close(votes[l].double(), want[l], rtol=1e-5, atol=0.0)


def test_ties_take_the_lower_index_first():
    from sm3hip import ops
    g = torch.Generator(device=DEV).manual_seed(3)
    B, N, ld = 6, 3000, 3004
    # few distinct values: every k below cuts through a tie group
    S = torch.randint(0, 12, (B, ld), generator=g, device=DEV).float() / 12.0 - 0.25
    S[:, 5] = -0.0
    S[:, 9] = 0.0
    targets = _labels(g, N, [4]).to(torch.int32)
    for k in (1, 7, 200, 1000, 1024):
        scores = torch.empty(B, 4, device=DEV)
        idx = torch.empty(B, k, dtype=torch.int32, device=DEV)
        sim = torch.empty(B, k, device=DEV)
        ops.knn_vote(S, N, targets, [0, 4], k, 0.1, scores, idx, sim)
        want, widx, wval = _restate(S, N, targets, [4], k, 0.1)
        assert torch.equal(idx.long(), widx), k
        assert torch.equal(sim.double(), wval), k
        torch.testing.assert_close(scores.double(), want[0], rtol=1e-5, atol=0.0)
    # duplicated bank rows through the whole path
    from sm3hip.knn import KNNBank, knn_scores
    base = _features(g, 40, 64)
    pick = torch.randint(0, 40, (900,), generator=g, device=DEV)
    bank_f, q = base[pick], _features(g, 5, 64)
    t = _labels(g, 900, [3])
    _, (idx, _) = knn_scores(q, bank_f, t, [3], k=100, temperature=0.07, neighbors=True)
    kb = KNNBank(bank_f, t, [3])
    Sg = torch.empty(5, kb.ld, device=DEV)
    kb.similarity(q, Sg)
    want = torch.sort(Sg[:, :900], dim=1, descending=True, stable=True).indices[:, :100]
    assert torch.equal(idx.long(), want)
    for b in range(5):  # the tied rows really are tied and come out in index order
        vals = Sg[b, idx[b].long()]
        same = vals[1:] == vals[:-1]
        assert bool(same.any()) and bool((idx[b, 1:][same] > idx[b, :-1][same]).all())


def test_repeated_calls_and_query_chunking_give_equal_bits():
    from sm3hip.knn import KNNBank, knn_scores
    g = torch.Generator(device=DEV).manual_seed(4)
    N, D, B = 20000, 256, 37
    bank = KNNBank(_features(g, N, D), _labels(g, N, DERM7PT_CLASSES), DERM7PT_CLASSES)
    q = _features(g, B, D)
    ref, (ri, rs) = knn_scores(q, bank, k=200, neighbors=True)
    again, (ai, as_) = knn_scores(q, bank, k=200, neighbors=True)
    for rows in (1, 3, 16):
        chunked, (ci, cs) = knn_scores(q, bank, k=200, neighbors=True, max_s_bytes=rows * 4 * bank.ld)
        assert all(torch.equal(a, b) for a, b in zip(ref, chunked)) and torch.equal(ri, ci) and torch.equal(rs, cs)
    assert all(torch.equal(a, b) for a, b in zip(ref, again)) and torch.equal(ri, ai) and torch.equal(rs, as_)
    # one query alone equals its row of the batch
    one = knn_scores(q[11:12].clone(), bank, k=200)
    assert all(torch.equal(a[11:12], b) for a, b in zip(ref, one))


def test_the_l_label_call_equals_l_single_label_calls():
    from sm3hip.knn import knn_scores
    g = torch.Generator(device=DEV).manual_seed(5)
    N, D, B = 7000, 128, 20
    bank_f, q = _features(g, N, D), _features(g, B, D)
    t = _labels(g, N, DERM7PT_CLASSES)
    votes = knn_scores(q, bank_f, t, DERM7PT_CLASSES, k=200)
    for l, c in enumerate(DERM7PT_CLASSES):
        (single,) = knn_scores(q, bank_f, t[:, l].contiguous(), c, k=200)
        assert torch.equal(votes[l], single), l


def test_out_of_range_arguments_raise_and_launch_nothing():
    import ctypes as C
    from sm3hip import _lib, ops
    from sm3hip.knn import knn_scores
    g = torch.Generator(device=DEV).manual_seed(6)
    B, N = 4, 100
    S = torch.randn(B, N, generator=g, device=DEV)
    targets = torch.zeros(N, 1, dtype=torch.int32, device=DEV)
    scores = torch.full((B, 5), 7.0, device=DEV)
    for k in (0, 101):
        with pytest.raises(ValueError):
            ops.knn_vote(S, N, targets, [0, 5], k, 0.07, scores)
    with pytest.raises(ValueError):
        ops.knn_vote(S, N, targets, [0, 5], 5, 0.0, scores)
    with pytest.raises(ValueError):
        ops.knn_vote(S, N, targets, [0, 257], 5, 0.07, torch.full((B, 257), 7.0, device=DEV))
    with pytest.raises(ValueError):
        ops.knn_vote(S, N, torch.zeros(N, 17, dtype=torch.int32, device=DEV), list(range(18)), 5, 0.07,
                     torch.full((B, 17), 7.0, device=DEV))
    with pytest.raises(ValueError):
        ops.knn_vote(S, N, targets.long(), [0, 5], 5, 0.07, scores)
    with pytest.raises(ValueError):
        knn_scores(S, torch.randn(2000, N, device=DEV), torch.zeros(2000, dtype=torch.int64, device=DEV), 5, k=1025)
    with pytest.raises(ValueError):
        knn_scores(S, torch.randn(50, N, device=DEV), torch.full((50,), 5, dtype=torch.int64, device=DEV), 5, k=5)
    lib = _lib.load()
    off = (C.c_int32 * 2)(0, 5)
    for k in (0, 101, 1025):
        assert lib.sm3_knn_vote(ops._ptr(S), B, N, N, ops._ptr(targets), 1, off, k, 0.07, ops._ptr(scores), None, None,
                                ops._stream()) == -1
    torch.cuda.synchronize()
    assert bool((scores == 7.0).all())


class _Encoder(torch.nn.Module):
    """A resnet18 encoder on the HIP engine whose output is the pooled feature (fc = Identity)."""

    def __init__(self):
        super().__init__()
        from src.models.resnet import resnet18
        self.net = resnet18(weights=None)
        self.net.fc = torch.nn.Identity()

    def forward(self, x):
        return self.net(x)


def test_on_validation_epoch_end_equals_the_restated_accuracy():
    from src.models.evaluator import KNNOnlineEvaluator
    torch.manual_seed(0)
    model = _Encoder().to(DEV)
    g = torch.Generator().manual_seed(7)
    C = 3
    train = [(torch.randn(8, 3, 64, 64, generator=g), torch.randint(0, C, (8,), generator=g)) for _ in range(3)]
    val = [(torch.randn(6, 3, 64, 64, generator=g), torch.randint(0, C, (6,), generator=g)) for _ in range(2)]
    ev = KNNOnlineEvaluator(train, val, C, k=10, temperature=0.1)
    acc = ev.on_validation_epoch_end(model)
    with torch.no_grad():
        f = lambda x: torch.nn.functional.normalize(model(x.to(DEV)).double(), dim=1)
        bank = torch.cat([f(x) for x, _ in train])
        tb = torch.cat([y for _, y in train]).to(DEV)
        q = torch.cat([f(x) for x, _ in val])
        tq = torch.cat([y for _, y in val]).to(DEV)
    votes, _, _ = _restate(q @ bank.T, bank.shape[0], tb, [C], 10, 0.1)
    want = float((votes[0].argsort(dim=1, descending=True, stable=True)[:, 0] == tq).double().mean())
    assert 0.0 <= acc <= 1.0 and abs(acc - want) < 1e-12, (acc, want)


def _tool(name):
    spec = importlib.util.spec_from_file_location("sm3_knn_gpu_" + name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _check_tool_output(stat, log_path, k, T):
    from sm3hip.knn import KNNBank
    from sm3hip.metrics import auc_avg
    saved = torch.load(os.path.join(log_path, "knn_predictions.pt"), map_location="cpu", weights_only=False)
    bank_f, bank_t = saved["bank_features"].to(DEV), saved["bank_targets"].to(DEV)
    q, tq = saved["query_features"].to(DEV), saved["targets"].to(DEV)
    kb = KNNBank(bank_f, bank_t, DERM7PT_CLASSES)
    S = torch.empty(q.shape[0], kb.ld, device=DEV)
    kb.similarity(torch.nn.functional.pad(q, (0, kb.Dp - kb.D)), S)
    votes, _, _ = _restate(S, kb.N, bank_t, DERM7PT_CLASSES, k, T)
    for got, want in zip(saved["votes"], votes):
        torch.testing.assert_close(got.to(DEV).double(), want, rtol=1e-5, atol=0.0)
    _, avg = auc_avg([(v / v.sum(dim=1, keepdim=True)).log() for v in votes], tq)
    assert abs(float(avg) - stat["AUC_AVG"]) < 1e-6 and saved["AUC_AVG"] == stat["AUC_AVG"], (float(avg), stat["AUC_AVG"])
    assert math.isfinite(stat["AUC_AVG"]) and stat["pairs_per_s"] > 0
    return saved


def test_backbone_knn_on_synthetic_data(tmp_path, capsys):
    bk = _tool("backbone_knn")
    stat = bk.main(["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "-b", "4", "--img-sz", "64", "64",
                    "--steps-per-epoch", "3", "--val-steps", "2", "--knn-k", "5", "--knn-t", "0.1", "--save-features",
                    "--log-path", str(tmp_path)])
    out = capsys.readouterr().out
    assert "AUC_AVG" in out and "bank 12 queries 8" in out, out
    saved = _check_tool_output(stat, str(tmp_path), 5, 0.1)
    assert saved["bank_size"] == 12 and saved["query_features"].shape == (8, 1024)


def _write_tree(root, seed=0):
    """A derm7pt-shaped directory: the fixture's metadata with small PNG images (derm 120 x 160, clinic 100 x 140)."""
    g = np.random.default_rng(seed)
    meta = pd.read_csv(os.path.join(META, "meta.csv"))
    derm, clinic = [], []
    for i in range(len(meta)):
        os.makedirs(root / "images" / f"Case{i:03d}", exist_ok=True)
        for kind, names, (h, w) in (("d", derm, (120, 160)), ("c", clinic, (100, 140))):
            name = f"Case{i:03d}/{kind}{i:03d}.png"
            Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / "images" / name)
            names.append(name)
    meta["derm"], meta["clinic"] = derm, clinic
    meta.to_csv(root / "meta.csv", index=False)
    for f in ("train_indexes.csv", "valid_indexes.csv", "test_indexes.csv"):
        pd.read_csv(os.path.join(META, f)).to_csv(root / f, index=False)
    return root


def test_backbone_knn_on_a_derm7pt_tree(tmp_path, capsys):
    from src.utils.data.datasets import read_split
    tree = _write_tree(tmp_path / "7PC")
    bk = _tool("backbone_knn")
    stat = bk.main(["--data-name", "SevenPCBaseDataset", "--data-path", str(tree), "-j", "4",
                    "--mean", "0.7833", "0.6712", "0.6026", "--std", "0.2139", "0.2472", "0.2571",
                    "-a", "resnet18", "-b", "6", "--img-sz", "64", "64", "--knn-k", "5", "--save-features",
                    "--log-path", str(tmp_path / "knn")])
    saved = _check_tool_output(stat, str(tmp_path / "knn"), 5, 0.07)
    assert torch.equal(saved["targets"], read_split(str(tree), "test")[2])   # the test split's labels, in order
    assert saved["bank_size"] == len(read_split(str(tree), "train")[2]) == stat["bank"]
