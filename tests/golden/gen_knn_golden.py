"""Hand-run generator of knn_ref.npz (never imported by a test).

Calls the reference's own ``KNNOnlineEvaluator.predict`` (src/models/evaluator.py) on CPU, in float32, on seeded
clustered unit-norm features, and stores per case the queries, the bank, the targets and the reference's ``pred_labels``,
with the constructor's defaults (k, temperature) read from the reference's signature.  A draw is rejected when it has a
near-tie (relative gap below 1e-4) between the k-th and (k+1)-th similarity of a row or between two non-zero class scores,
or when the reference's order of the zero-score classes is not the lower-class-first one, so that the golden does not depend
on the order in which sums are formed or ties broken.

    SM3_REFERENCE=<reference checkout> python tests/golden/gen_knn_golden.py
"""
import importlib.util
import inspect
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SM3_REFERENCE")
GAP = 1e-4

# name: (B, N, D, k, classes, temperature)
CASES = {
    "k1": (8, 300, 64, 1, 5, 0.07),
    "k7": (8, 300, 64, 7, 5, 0.07),
    "k200_n450": (16, 450, 128, 200, 5, 0.07),
    "kN": (6, 96, 96, 96, 2, 0.1),
    "b1": (1, 250, 32, 7, 2, 0.07),
    "n333_d40": (12, 333, 40, 20, 5, 0.5),
}


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_evaluator", os.path.join(REF, "src", "models", "evaluator.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.KNNOnlineEvaluator


def draw(g, B, N, D, C):
    centers = torch.randn(C, D, generator=g, dtype=torch.float64)
    targets = torch.randint(0, C, (N,), generator=g)
    qcls = torch.randint(0, C, (B,), generator=g)
    bank = centers[targets] * 0.6 + torch.randn(N, D, generator=g, dtype=torch.float64)
    query = centers[qcls] * 0.6 + torch.randn(B, D, generator=g, dtype=torch.float64)
    bank = (bank / bank.norm(dim=1, keepdim=True)).float()
    query = (query / query.norm(dim=1, keepdim=True)).float()
    return query, bank, targets


def well_separated(query, bank, targets, C, k, T, pred):
    S = (query @ bank.T).double()
    srt = S.sort(dim=1, descending=True).values
    if k < S.shape[1]:
        a, b = srt[:, k - 1], srt[:, k]
        if bool(((a - b).abs() < GAP * a.abs().clamp_min(1e-3)).any()):
            return False
    idx = S.topk(k, dim=1).indices
    w = torch.exp(S.gather(1, idx) / T)
    scores = torch.zeros(S.shape[0], C, dtype=torch.float64).scatter_add_(1, targets[idx], w)
    for row in scores:
        nz = row[row > 0].sort().values
        if len(nz) > 1 and bool(((nz[1:] - nz[:-1]) < GAP * nz[1:]).any()):
            return False
    # the ranking the contract fixes: descending, equal (zero) scores lower class first
    return torch.equal(pred, scores.argsort(dim=1, descending=True, stable=True))


def main():
    if not REF:
        raise SystemExit("set SM3_REFERENCE to the reference checkout")
    Ref = load_reference()
    sig = inspect.signature(Ref.__init__).parameters
    out = {"default_k": np.int64(sig["k"].default), "default_temperature": np.float64(sig["temperature"].default),
           "cases": np.array(list(CASES))}
    g = torch.Generator().manual_seed(20261015)
    for name, (B, N, D, k, C, T) in CASES.items():
        for attempt in range(200):
            query, bank, targets = draw(g, B, N, D, C)
            ev = Ref(None, None, C, k=k, temperature=T)
            pred = ev.predict(query, bank, targets)
            if well_separated(query, bank, targets, C, k, T, pred):
                break
        else:
            raise SystemExit(f"{name}: no well-separated draw")
        out.update({f"{name}_query": query.numpy(), f"{name}_bank": bank.numpy(), f"{name}_targets": targets.numpy(),
                    f"{name}_pred_labels": pred.numpy(), f"{name}_meta": np.array([k, C], dtype=np.int64),
                    f"{name}_temperature": np.float64(T)})
        print(f"{name}: B={B} N={N} D={D} k={k} C={C} T={T} after {attempt + 1} draw(s)")
    np.savez_compressed(os.path.join(HERE, "knn_ref.npz"), **out)


if __name__ == "__main__":
    main()
