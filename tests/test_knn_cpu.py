"""CPU: the weighted kNN evaluator's surface -- KNNOnlineEvaluator's constructor against the reference's (golden), the
argument checks of sm3_knn_vote / ops.knn_vote / knn_scores, which all run before any launch, and backbone_knn's command
line.  No GPU use."""
import ctypes as C
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")


def test_constructor_signature_and_defaults_match_the_reference(golden_dir):
    from src.models.evaluator import KNNOnlineEvaluator
    g = np.load(os.path.join(golden_dir, "knn_ref.npz"))
    params = inspect.signature(KNNOnlineEvaluator.__init__).parameters
    assert list(params) == ["self", "train_dataloader", "val_dataloader", "n_classes", "k", "temperature"]
    assert params["k"].default == int(g["default_k"]) == 200
    assert params["temperature"].default == float(g["default_temperature"]) == 0.07
    ev = KNNOnlineEvaluator("train", "val", 7)
    assert (ev.train_dataloader, ev.val_dataloader, ev.num_classes, ev.k, ev.temperature) == ("train", "val", 7, 200, 0.07)


def _abi_call(lib, B=4, N=100, ld=100, L=1, offs=(0, 5), k=10, T=0.07, S=1, targets=1, scores=1):
    off = (C.c_int32 * len(offs))(*offs)
    return lib.sm3_knn_vote(S, B, N, ld, targets, L, off, k, T, scores, None, None, None)


def test_abi_rejects_bad_arguments_before_any_launch():
    from sm3hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    bad = [dict(k=0), dict(k=101), dict(N=2000, ld=2000, k=1025), dict(L=0), dict(L=17, offs=tuple(range(18))),
           dict(offs=(0, 257)), dict(L=2, offs=(0, 200, 257)), dict(L=2, offs=(0, 3, 3)), dict(offs=(1, 5)),
           dict(T=0.0), dict(T=float("inf")), dict(T=float("nan")), dict(S=None), dict(targets=None), dict(scores=None),
           dict(B=0), dict(ld=99), dict(B=2 ** 31), dict(N=2 ** 31, ld=2 ** 31, k=5)]
    for kw in bad:
        assert _abi_call(lib, **kw) == -1, kw


def _cpu_args(B=3, N=50, L=1, classes=(5,)):
    offs = [0]
    for c in classes:
        offs.append(offs[-1] + c)
    S = torch.zeros(B, N)
    targets = torch.zeros(N, L, dtype=torch.int32)
    scores = torch.zeros(B, offs[-1])
    return S, targets, offs, scores


@pytest.mark.parametrize("k", [0, 51, 1025])
def test_ops_knn_vote_rejects_bad_k(k):
    from sm3hip import ops
    N = 2000 if k == 1025 else 50
    S, targets, offs, scores = _cpu_args(N=N)
    with pytest.raises(ValueError, match="k = "):
        ops.knn_vote(S, N, targets, offs, k, 0.07, scores)


def test_ops_knn_vote_rejects_bad_labels_classes_and_cpu_tensors():
    from sm3hip import ops
    S, targets, offs, scores = _cpu_args(L=17, classes=(2,) * 17)
    with pytest.raises(ValueError, match="labels"):
        ops.knn_vote(S, 50, targets, offs, 5, 0.07, scores)
    S, targets, offs, scores = _cpu_args(L=2, classes=(200, 57))
    with pytest.raises(ValueError, match="classes over all labels"):
        ops.knn_vote(S, 50, targets, offs, 5, 0.07, scores)
    S, targets, offs, scores = _cpu_args()
    with pytest.raises(ValueError, match="GPU"):
        ops.knn_vote(S, 50, targets, offs, 5, 0.07, scores)


def test_knn_scores_rejects_bad_arguments_and_cpu_tensors():
    from sm3hip.knn import knn_scores
    q, bank = torch.randn(4, 64), torch.randn(50, 64)
    t = torch.zeros(50, dtype=torch.int64)
    for k in (0, 51):
        with pytest.raises(ValueError, match="k = "):
            knn_scores(q, bank, t, 5, k=k)
    big = torch.randn(2000, 64)
    with pytest.raises(ValueError, match="k = "):
        knn_scores(q, big, torch.zeros(2000, dtype=torch.int64), 5, k=1025)
    with pytest.raises(ValueError, match="labels"):
        knn_scores(q, bank, torch.zeros(50, 17, dtype=torch.int64), [2] * 17, k=5)
    with pytest.raises(ValueError, match="at most 256"):
        knn_scores(q, bank, torch.zeros(50, 2, dtype=torch.int64), [200, 57], k=5)
    with pytest.raises(ValueError, match="GPU"):
        knn_scores(q, bank, t, 5, k=5)


def test_predict_rejects_cpu_tensors():
    from src.models.evaluator import KNNOnlineEvaluator
    ev = KNNOnlineEvaluator(None, None, 5, k=5)
    with pytest.raises(ValueError, match="GPU"):
        ev.predict(torch.randn(4, 64), torch.randn(50, 64), torch.zeros(50, dtype=torch.int64))


def _tool(name):
    spec = importlib.util.spec_from_file_location("sm3_knn_cpu_" + name, os.path.join(TOOLS, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_backbone_knn_parser_takes_a_run_sh_line_and_the_knn_flags():
    bk = _tool("backbone_knn")
    line = ["-a", "resnet50", "--data-name", "SevenPCBaseDataset", "--data-path", "./data/7PC",
            "--mean", "0.7833", "0.6712", "0.6026", "--std", "0.2139", "0.2472", "0.2571",
            "--epochs", "50", "-b", "128", "-lr", "1e-3", "-j", "4", "--img-sz", "224", "224", "--num-labels", "8",
            "--pretrain-path", "logs/ckp_49.pth", "--finetune", "fc", "--log-path", "logs/test_49",
            "--proj-name", "sm3_r50_backbone_eval", "--amp"]
    args = bk.get_parser().parse_args(line)
    assert (args.knn_k, args.knn_t, args.random_features) == (200, 0.07, None)
    assert args.arch == "resnet50" and args.batch_size == 128 and args.img_sz == [224, 224] and args.amp
    args = bk.get_parser().parse_args(line + ["--knn-k", "50", "--knn-t", "0.1"])
    assert (args.knn_k, args.knn_t) == (50, 0.1)
    # the helpers are eval_cli's own, not copies
    import eval_cli
    assert bk.eval_cli is eval_cli and bk.eval_cli.load_ssl_backbones is eval_cli.load_ssl_backbones
