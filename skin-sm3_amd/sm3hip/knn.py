"""Weighted k-nearest-neighbour scores on the HIP engine -- the hot path of KNNOnlineEvaluator (src/models/evaluator.py).

    S = query . bank^T      the exact-f32 gather-GEMM (sm3_conv_gather_gemm), as the trainer's global negatives use it
    votes = sm3_knn_vote(S)  per query: the k largest similarities, exp(s / T), summed per class of every label

Nothing is normalised here (the reference's `predict` does not normalise either).  The GEMM needs the feature width D to be
a multiple of 32 and the bank size a multiple of 4: a bank that is not is zero-padded once, when the KNNBank is built (zero
columns leave every dot product unchanged; the padded bank rows are not among the N columns the vote reads).  A bank over
2 GiB is multiplied in column blocks that write straight into their columns of S; the queries are taken in chunks that keep
S under `max_s_bytes`.  Rows of S do not depend on the chunking, nor votes on the grid: the scores of a query are the same
bits however the queries are batched.
"""
import torch

from . import ops
from ._lib import SM3_F32

_GEMM_MAX_BYTES = 1 << 31  # per operand; the gather-GEMM addresses an operand with a 32-bit offset below 3 GiB


def _ceil(a, b):
    return -(-a // b)


def _require_gpu_f32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor (the SM3 HIP path has no CPU fallback)")
    if t.dtype != torch.float32 or t.dim() != 2:
        raise ValueError(f"{name} must be a 2-D float32 tensor, got {tuple(t.shape)} {t.dtype}")


class KNNBank:
    """A feature bank [N, D] with its targets, ready for knn_scores: targets checked against num_classes once, here."""

    def __init__(self, bank, targets, num_classes, block_bytes=_GEMM_MAX_BYTES):
        if bank.dim() != 2 or bank.shape[0] < 1 or bank.shape[1] < 1:
            raise ValueError(f"bank must be a non-empty [N, D] tensor, got {tuple(bank.shape)}")
        N, D = bank.shape
        t2 = targets.reshape(N, 1) if targets.dim() == 1 else targets
        if t2.dim() != 2 or t2.shape[0] != N:
            raise ValueError(f"targets {tuple(targets.shape)} do not match a bank of {N} rows")
        L = t2.shape[1]
        classes = [int(num_classes)] if isinstance(num_classes, int) else [int(c) for c in num_classes]
        if not 1 <= L <= ops.KNN_MAX_LABELS or len(classes) != L:
            raise ValueError(f"{L} target columns, {len(classes)} class counts: 1 to {ops.KNN_MAX_LABELS} labels")
        if min(classes) < 1 or sum(classes) > ops.KNN_MAX_CLASSES:
            raise ValueError(f"class counts {classes}: each at least 1, at most {ops.KNN_MAX_CLASSES} over all labels")
        _require_gpu_f32(bank, "bank")
        if not targets.is_cuda:
            raise ValueError("targets must be a GPU tensor (the SM3 HIP path has no CPU fallback)")
        if targets.dtype.is_floating_point or targets.dtype == torch.bool:
            raise ValueError(f"targets must hold integer classes, got {targets.dtype}")
        hi = torch.tensor(classes, device=bank.device, dtype=t2.dtype)
        if not bool(((t2 >= 0) & (t2 < hi)).all()):
            raise ValueError(f"a target lies outside its label's classes {classes}")
        self.N, self.D, self.L, self.classes = N, D, L, classes
        self.offsets = [0]
        for c in classes:
            self.offsets.append(self.offsets[-1] + c)
        self.targets = t2.to(torch.int32).contiguous()
        self.Dp = _ceil(D, ops.K_CHUNK[SM3_F32]) * ops.K_CHUNK[SM3_F32]
        # column blocks of equal width Nc (a multiple of 4) under block_bytes each; S has ld = blocks * Nc columns
        cap = max(4, (block_bytes // (4 * self.Dp)) // 4 * 4)
        Np = _ceil(N, 4) * 4
        self.blocks = _ceil(Np, cap)
        self.Nc = _ceil(_ceil(Np, self.blocks), 4) * 4
        self.ld = self.blocks * self.Nc
        if self.ld == N and self.Dp == D and bank.is_contiguous():
            self.weights = bank
        else:
            self.weights = torch.zeros(self.ld, self.Dp, dtype=torch.float32, device=bank.device)
            self.weights[:N, :D].copy_(bank)

    def similarity(self, query, S):
        """S[:B, :ld] = query . bank^T for a [B, Dp] query chunk (the columns past N multiply zero rows)."""
        B = query.shape[0]
        for g in range(self.blocks):
            d = ops.fwd_desc(SM3_F32, B, 1, 1, self.Dp, self.Nc, 1, 1, 0)
            d.Wout, d.oox = self.blocks, g  # block g writes columns [g * Nc, (g + 1) * Nc) of the ld-wide rows
            ops.conv_gemm(d, query, self.weights[g * self.Nc:(g + 1) * self.Nc], S, None, None)


def knn_scores(query, bank, targets=None, num_classes=None, k=200, temperature=0.07, neighbors=False,
               max_s_bytes=1 << 30):
    """Per-label vote tensors [B, C_l] of the weighted kNN classifier: votes[l][b, c] = sum of exp(s / T) over the k bank
    rows most similar to query b (s = <query b, bank row>) whose class for label l is c.

    bank: a KNNBank, or a [N, D] float32 GPU tensor with targets [N] / [N, L] and num_classes (int / L ints).
    neighbors=True also returns (indices [B, k] int32, similarities [B, k]) in rank order, equal similarities lower index
    first."""
    N = bank.N if isinstance(bank, KNNBank) else bank.shape[0]
    if not 1 <= k <= min(N, ops.KNN_MAX_K):
        raise ValueError(f"k = {k} outside [1, min(N = {N}, {ops.KNN_MAX_K})]")
    if not temperature > 0:
        raise ValueError("temperature must be positive")
    if not isinstance(bank, KNNBank):
        bank = KNNBank(bank, targets, num_classes)
    _require_gpu_f32(query, "query")
    B, D = query.shape
    if B < 1:
        raise ValueError("no queries")
    if D != bank.D:
        raise ValueError(f"query width {D} != bank width {bank.D}")
    dev = query.device
    scores = torch.empty(B, bank.offsets[-1], dtype=torch.float32, device=dev)
    idx = torch.empty(B, k, dtype=torch.int32, device=dev) if neighbors else None
    sim = torch.empty(B, k, dtype=torch.float32, device=dev) if neighbors else None
    rows = max(1, min(B, max_s_bytes // (4 * bank.ld), _GEMM_MAX_BYTES // (4 * bank.Dp)))
    S = torch.empty(rows, bank.ld, dtype=torch.float32, device=dev)
    for b0 in range(0, B, rows):
        q = query[b0:b0 + rows]
        n = q.shape[0]
        q = q.contiguous() if bank.Dp == D else torch.nn.functional.pad(q, (0, bank.Dp - D))
        Sc = S[:n]
        bank.similarity(q, Sc)
        ops.knn_vote(Sc, bank.N, bank.targets, bank.offsets, k, temperature, scores[b0:b0 + n],
                     None if idx is None else idx[b0:b0 + n], None if sim is None else sim[b0:b0 + n])
    votes = [scores[:, bank.offsets[l]:bank.offsets[l + 1]] for l in range(bank.L)]
    return (votes, (idx, sim)) if neighbors else votes


def normalize(feat):
    """Rows scaled to unit L2 norm on the HIP kernel (sm3_normalize_rows): the F.normalize of the reference's feature bank."""
    _require_gpu_f32(feat, "features")
    feat = feat.contiguous()
    out = torch.empty_like(feat)
    inv = torch.empty(feat.shape[0], dtype=torch.float32, device=feat.device)
    ops.normalize_rows(feat, out, inv)
    return out
