"""Test helper of the multi-label head edge suites (test_heads_train_edges_gpu.py, test_heads_ce_kmeans_edges_gpu.py,
test_heads_infer_edges_gpu.py): case tables, mask probes, fp64 references, torch-fp32 restatements and bounds of the
kernels in csrc/heads_train.hip and csrc/heads.hip.  CPU only: nothing here touches the library.

Bounds, each stated once (below):
  * exact (== on bits, +0 == -0 as exact_inputs.same) wherever a result is one fp32 operation, a copy or an integer sum;
  * the project's own unit-scale figures (tests/test_inference_model.py, tests/test_mlc.py): UNIT_OUT, UNIT_LOSS,
    UNIT_DLOGITS, UNIT_CENT, UNIT_GRAD_NORM;
  * for everything else derived(): 8 x the worst error of the torch-fp32 restatement of the same formula against the
    fp64 reference over the cases of the regime, in the measure rel_err() (error over max|ref| + |ref|), never below
    DERIVED_FLOOR.  test_head_refs_cpu.py holds every restatement to a quarter of the bound derived from it.
Dropout masks are never computed here: the GPU tests read them from the forward kernels with the probe operands below.
The derived bounds need some mask on the CPU and use a seeded Bernoulli one (bernoulli_mask): the arithmetic is the
same for every mask of that keep rate."""
import functools
import math

import numpy as np
import torch

from edge_inputs import HALF_ULP, f32, record, worst_ratio  # noqa: F401  (re-exported)
from exact_inputs import Guarded, draw, need_exact, quantum, same  # noqa: F401

F64, F32 = torch.float64, torch.float32
EPS = 1e-5
PS = [0.0, 0.1, 0.5]
EINVAL = -1

UNIT_OUT = 1e-5          # attention and LayerNorm outputs, absolute (tests/test_inference_model.py)
UNIT_LOSS = 1e-5         # tests/test_mlc.py
UNIT_DLOGITS = 1e-7      # tests/test_mlc.py, at k / T = 1 / (192 * 0.7): see ce_dlogits_unit()
UNIT_CENT = 1e-5         # tests/test_mlc.py
UNIT_GRAD_NORM = 2e-4    # |got - ref| / |ref| of a whole gradient (tests/test_mlc.py)
DERIVED_FACTOR = 8.0
RESTATE_SHARE = 0.25
DERIVED_FLOOR = 8.0 * 2.0 ** -24   # one fp32 rounding of the largest element, times the same factor


def gen(seed):
    return torch.Generator().manual_seed(seed)


def scale64(p):
    """1 / (1 - f32(p)) in fp64: p crosses the C ABI as a float."""
    return 1.0 / (1.0 - f32(p)) if p > 0 else 1.0


def scale32(p):
    """fl(1 / (1 - p)) as the kernels compute it (two correctly rounded fp32 operations); 1 for p = 0."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def rel_err(got, ref, scale=None):
    """max |got - ref| / (scale + |ref|): the error against the size of what entered the result.  scale: a number or a
    tensor that broadcasts against ref; None: max|ref|, the tensor's own scale.  inf for a non-finite result."""
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    if ref.numel() == 0:
        return 0.0
    s = ref.abs().max() if scale is None else torch.as_tensor(scale, dtype=F64)
    den = s + ref.abs()
    err = (got - ref).abs()
    bad = (den == 0) & (err > 0)
    if bool(bad.any()):
        return math.inf
    return float((err / den.clamp_min(1e-300)).max())


def abs_err(got, ref):
    got = got.double()
    return float((got - ref.double()).abs().max()) if bool(torch.isfinite(got).all()) else math.inf


def norm_err(got, ref):
    return float((got.double() - ref.double()).norm() / (ref.double().norm() + 1e-30))


def half_limit(ref, base, dtype):
    """base (absolute) plus one rounding of a 16-bit store, element-wise."""
    return base + ref.double().abs() * HALF_ULP[dtype]


def bernoulli_mask(shape, p, seed):
    return torch.ones(shape, dtype=torch.bool) if p <= 0 else torch.rand(shape, generator=gen(seed)) >= p


def keep_rate_ok(mask, p):
    """(|rate - (1 - p)|, 5 sigma) over the mask's elements."""
    n = mask.numel()
    return abs(float(mask.double().mean()) - (1.0 - f32(p))), 5.0 * math.sqrt(p * (1.0 - p) / n)


def differ_ok(m0, m1, p):
    """(|share of differing positions - 2p(1-p)|, 5 sigma) of two independent masks."""
    n = m0.numel()
    q = 2.0 * p * (1.0 - p)
    return abs(float((m0 != m1).double().mean()) - q), 5.0 * math.sqrt(q * (1.0 - q) / n)


# ------------------------------------------------------------------------------------------------------------------------
# row layouts: logical [B, S, W] <-> the [B * S, W] rows the kernels address (label_major: row s * B + b, else b * S + s)
# ------------------------------------------------------------------------------------------------------------------------
def to_rows(x, label_major):
    B, S, W = x.shape
    return (x.permute(1, 0, 2) if label_major else x).reshape(B * S, W).contiguous()


def from_rows(r, B, S, label_major):
    W = r.shape[-1]
    return r.reshape(S, B, W).permute(1, 0, 2).contiguous() if label_major else r.reshape(B, S, W)


# ------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------
ATT_CASES = [(1, 64, 1), (1, 4096, 8), (8, 512, 1), (8, 256, 4), (8, 8, 8), (5, 24, 8), (3, 6, 2), (7, 520, 8), (8, 64, 8)]
ATT_BS = [1, 3]
ATT_REGIMES = ["unit", "peaked", "tied"]
ATT_MASK_CASES = [(8, 64, 8), (5, 24, 8), (3, 6, 2), (8, 256, 4)]   # the probe costs S launches: the cases with S > 1


@functools.lru_cache(maxsize=None)
def att_case(S, D, nhead, B, regime):
    """(qkv [B, S, 3D], dout [B, S, D]) fp32.  unit: scores of order +-3; peaked: max |score| 30 to 60, softmax near
    one-hot; tied: Q = 0."""
    g = gen(S * 100003 + D * 17 + nhead * 5 + B)
    hd = D // nhead
    q = torch.randn(B, S, D, generator=g, dtype=F64)
    k = torch.randn(B, S, D, generator=g, dtype=F64)
    v = torch.randn(B, S, D, generator=g, dtype=F64)
    dout = torch.randn(B, S, D, generator=g, dtype=F64)
    sc = torch.einsum("bihd,bjhd->bhij", q.view(B, S, nhead, hd), k.view(B, S, nhead, hd)) / math.sqrt(hd)
    top = float(sc.abs().max())
    if regime == "tied":
        return torch.cat([q * 0, k, v], 2).float(), dout.float()
    f = math.sqrt({"unit": 3.0, "peaked": 45.0}[regime] / top)
    return torch.cat([q * f, k * f, v], 2).float(), dout.float()


def att_scores(qkv, nhead):
    B, S, D3 = qkv.shape
    D = D3 // 3
    hd = D // nhead
    q, k = qkv[..., :D].double().view(B, S, nhead, hd), qkv[..., D:2 * D].double().view(B, S, nhead, hd)
    return torch.einsum("bihd,bjhd->bhij", q, k) / math.sqrt(hd)


def att_apply(qkv, dout, nhead, mask, p, dt):
    """softmax(Q K^T / sqrt(hd)) with dropout mask [B, nhead, S, S] (None: no dropout) times V, and its gradient, by torch
    autograd in `dt` (fp64: the reference; fp32: the restatement).  -> out [B, S, D], dqkv [B, S, 3D]"""
    B, S, D3 = qkv.shape
    D = D3 // 3
    hd = D // nhead
    x = qkv.to(dt).clone().requires_grad_(True)
    q, k, v = (x[..., i * D:(i + 1) * D].reshape(B, S, nhead, hd) for i in range(3))
    sc = torch.einsum("bihd,bjhd->bhij", q, k) * torch.tensor(1.0 / math.sqrt(hd), dtype=dt)
    pr = torch.softmax(sc, -1)
    if mask is not None and p > 0:
        sc_ = torch.tensor(scale64(p) if dt == F64 else scale32(p), dtype=dt)
        pr = pr * mask.to(dt) * sc_
    out = torch.einsum("bhij,bjhd->bihd", pr, v).reshape(B, S, D)
    if dout is None:
        return out.detach(), None
    out.backward(dout.to(dt))
    return out.detach(), x.grad


def att_probe_qkv(B, S, D, jp, mag=1.0):
    """Q = K = 0, V = mag in token jp and 0 elsewhere: out[b, i, h*hd + d] != 0 <=> (b, h, i, jp) is kept."""
    qkv = torch.zeros(B, S, 3 * D)
    qkv[:, jp, 2 * D:] = mag
    return qkv


def att_mask_from_probe(outs, nhead):
    """outs: S tensors [B, S, D] (launch jp) -> mask [B, nhead, S(i), S(j)]; every d of a head must agree."""
    B, S, D = outs[0].shape
    hd = D // nhead
    cols = []
    for o in outs:
        nz = (o != 0).view(B, S, nhead, hd)
        assert bool((nz == nz[..., :1]).all()), "probe: the columns of one head disagree"
        cols.append(nz[..., 0].permute(0, 2, 1))       # [B, nhead, S(i)]
    return torch.stack(cols, -1)


# ------------------------------------------------------------------------------------------------------------------------
# add-LayerNorm
# ------------------------------------------------------------------------------------------------------------------------
LN_DS = [1, 2, 63, 64, 65, 1000, 1024, 1025, 4096]
LN_ROWS = [1, 3, 4, 5]
LN_INFER_DS = [1, 63, 64, 65, 1000, 1024]
LN_REGIMES = ["unit", "offset", "const"]
LN_CONST = 1.5   # exactly representable; a + b = 1.5 in every element of a constant row


@functools.lru_cache(maxsize=None)
def ln_case(rows, D, regime):
    """(a, b [rows, D], gamma, beta [D], dout [rows, D]) fp32.  offset: rows with mean 1e3 and std 0.1 (a one-pass variance
    loses them); const: every row a + b = LN_CONST (with p = 0)."""
    g = gen(rows * 7919 + D)
    a = torch.randn(rows, D, generator=g)
    b = torch.randn(rows, D, generator=g)
    if regime == "offset":
        a = 1e3 + 0.1 * a
        b = 0.1 * b
    elif regime == "const":
        a = torch.full((rows, D), 1.0)
        b = torch.full((rows, D), LN_CONST - 1.0)
    gamma = 1 + 0.1 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    dout = torch.randn(rows, D, generator=g)
    return a, b, gamma, beta, dout


def ln_apply(a, b, gamma, beta, dout, mask, p, dt):
    """LayerNorm(a + dropout(b)) (two-pass biased variance, eps = f32(1e-5)) and its gradients by autograd in `dt`.
    b None: LayerNorm(a).  -> dict out, mean, rstd, xhat, da, db, dgamma, dbeta"""
    A = a.to(dt).clone().requires_grad_(True)
    G = gamma.to(dt).clone().requires_grad_(True)
    Bt = beta.to(dt).clone().requires_grad_(True)
    x = A
    Bb = None
    if b is not None:
        Bb = b.to(dt).clone().requires_grad_(True)
        bb = Bb
        if mask is not None and p > 0:
            bb = Bb * torch.tensor(scale64(p) if dt == F64 else scale32(p), dtype=dt) * mask.to(dt)
        x = A + bb
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(f32(EPS), dtype=dt))
    xhat = (x - mean) * rstd
    out = xhat * G + Bt
    r = dict(out=out.detach(), mean=mean.detach()[:, 0], rstd=rstd.detach()[:, 0], xhat=xhat.detach(),
             xabs=x.detach().abs().mean(1))          # the size of what entered the mean
    if dout is not None:
        out.backward(dout.to(dt))
        r.update(da=A.grad, db=None if Bb is None else Bb.grad, dgamma=G.grad, dbeta=Bt.grad)
    return r


def ln_mask_from_probe(out, stats):
    """a = 0, b = mag > 0, gamma = 1, beta = 0: a kept element is above its row's mean and a dropped one below it, so within
    a row out > 0 <=> kept.  A row whose outputs are all equal (exactly 0 when the row sum is exact) is all kept or all
    dropped, and its mean in `stats`, 0 or not, says which."""
    rows, D = out.shape
    flat = (out == out[:, :1]).all(1)
    m = out > 0
    m[flat] = (stats[flat, 0] != 0).unsqueeze(1).expand(-1, D)
    return m


# ------------------------------------------------------------------------------------------------------------------------
# bias-ReLU-dropout, colsum
# ------------------------------------------------------------------------------------------------------------------------
BRD_CASES = [(1, 1), (255, 1), (1, 255), (257, 1), (37, 7), (1, 257), (5, 64), (3, 100), (149797, 7)]  # (rows, N)
BRD_BIG = 4096 * 256 + 3
assert 149797 * 7 == BRD_BIG
FLT_MIN = 2.0 ** -126
ULP0 = 2.0 ** -149
BRD_TABLE = [0.0, -0.0, FLT_MIN, -FLT_MIN, ULP0, -ULP0, 1.0, -1.0, 0.37, -2.5, 3e-5, -3e-5, 1e4, -1e4]


@functools.lru_cache(maxsize=None)
def brd_case(rows, N):
    """(y [rows, N], bias [N], dhd [rows, N]) fp32.  bias is -0 in the even columns (x + -0 is x for every x, -0 included), where
    y + bias is the drawn entry of BRD_TABLE bit for bit, and 0.5 in the odd ones, where y = fl(entry - 0.5) and the tiny
    entries come back as +0."""
    g = gen(rows * 31 + N)
    tab = torch.tensor(BRD_TABLE, dtype=F64)
    want = tab[torch.randint(0, len(BRD_TABLE), (rows, N), generator=g)]
    bias = torch.zeros(N, dtype=F64)
    bias[1::2] = 0.5
    y = (want - bias).float()
    y[:, 0::2] = want[:, 0::2].float()         # keeps the sign of -0
    bias = bias.float()
    bias[0::2] = -0.0
    dhd = torch.randn(rows, N, generator=g)
    return y, bias, dhd


COLSUM_ROWS = [1, 3, 63, 64, 65, 4097]
COLSUM_NS = [1, 63, 64, 65, 130]


# ------------------------------------------------------------------------------------------------------------------------
# prototype heads
# ------------------------------------------------------------------------------------------------------------------------
# (S, D, Tn, l2, bias): every D with l2 on and off, every Tn, every S
HEAD_CASES = [(1, 1, 1, 0, 1), (1, 1, 21, 1, 0), (3, 7, 31, 0, 0), (3, 7, 32, 1, 1), (8, 8, 33, 1, 0), (8, 8, 21, 0, 1),
              (3, 31, 21, 1, 1), (8, 31, 256, 0, 0), (8, 32, 21, 0, 1), (3, 32, 33, 1, 0), (8, 33, 21, 1, 1), (3, 33, 1, 0, 0),
              (8, 512, 21, 1, 1), (8, 512, 32, 0, 0), (1, 4096, 21, 0, 1), (3, 4096, 31, 1, 0)]
HEAD_B = 3


def head_tokens(S, Tn):
    """token_of [Tn] int32, not monotone; with S >= 3 token 1 owns no prototype."""
    t = (torch.arange(Tn) * 5 + 2) % S
    if S >= 3:
        t = torch.where(t == 1, torch.full_like(t, S - 1), t)
    return t.to(torch.int32)


@functools.lru_cache(maxsize=None)
def head_case(S, D, Tn, l2, B=HEAD_B):
    """(x [B, S, D], W [Tn, D], bias [Tn], tok [Tn], dlogits [B, Tn]) fp32.  Rows of x have norms from 1e-3 to 1e3; with l2 and
    S >= 3, x[0, S - 1] is all zero."""
    g = gen(S * 1009 + D * 13 + Tn)
    x = torch.randn(B, S, D, generator=g, dtype=F64)
    x = x / x.norm(dim=2, keepdim=True).clamp_min(1e-30)
    sc = torch.logspace(-3, 3, B * S, dtype=F64)[torch.randperm(B * S, generator=g)]
    if S >= 3:   # the row that is zeroed under l2 gets the middle scale: the extremes stay in the table
        j = int((sc - sc.median()).abs().argmin())
        sc[[S - 1, j]] = sc[[j, S - 1]]
    x = x * sc.view(B, S, 1)
    if l2 and S >= 3:
        x[0, S - 1] = 0
    W = 0.1 * torch.randn(Tn, D, generator=g)
    bias = 0.1 * torch.randn(Tn, generator=g)
    gl = torch.randn(B, Tn, generator=g)
    return x.float(), W, bias, head_tokens(S, Tn), gl


def head_apply(x, W, bias, tok, gl, l2, dt):
    """-> logits [B, Tn], dx, dW, dbias by autograd in `dt` (F.normalize(eps = 1e-12) when l2)."""
    X = x.to(dt).clone().requires_grad_(True)
    Wt = W.to(dt).clone().requires_grad_(True)
    bt = None if bias is None else bias.to(dt).clone().requires_grad_(True)
    xn = torch.nn.functional.normalize(X, dim=-1, p=2, eps=1e-12) if l2 else X
    out = torch.einsum("btd,td->bt", xn[:, tok.long()], Wt)
    if bt is not None:
        out = out + bt
    if gl is None:
        return out.detach(), None, None, None
    out.backward(gl.to(dt))
    return out.detach(), X.grad, Wt.grad, None if bt is None else bt.grad


# ------------------------------------------------------------------------------------------------------------------------
# pseudo-label cross-entropy
# ------------------------------------------------------------------------------------------------------------------------
CE_WIDTHS = [[5, 3, 2, 3, 3, 3, 3, 2], [1, 5, 1, 2]]
# (widths, B).  The two width lists have 8 and 4 heads, so B * H is a multiple of 4: they run at B * H = 252, 256, 260, 2000
# (the 256-thread stride on either side of its boundary) and at B = 3; B * H = 1, 255 = 5 * 51 and 257 (a prime) need other
# head counts, and run with [3], with [1, 5, 1, 2] plus a three-class head, and with [3].
CE_SHAPES = [((3,), 1), ((1, 5, 1, 2, 3), 51), ((5, 3, 2, 3, 3, 3, 3, 2), 32), ((3,), 257), ((5, 3, 2, 3, 3, 3, 3, 2), 250),
             ((1, 5, 1, 2), 63), ((1, 5, 1, 2), 64), ((1, 5, 1, 2), 65), ((1, 5, 1, 2), 500), ((5, 3, 2, 3, 3, 3, 3, 2), 3)]
CE_TS = [1.0, 0.7, 0.1, 0.01]
CE_REGIMES = ["unit", "amp10", "dominant", "equal"]
CE_LOSS0 = 0.625


@functools.lru_cache(maxsize=None)
def ce_case(widths, B, regime, T):
    """(logits [B, Tn] fp32, targets [H, B] int64).  Targets hold the first and the last class of every head (B >= 2);
    dominant: one class leads its head by 200 T at least, the target is that class in the even rows."""
    widths = list(widths)
    H, Tn = len(widths), sum(widths)
    g = gen(B * 131 + Tn + int(T * 1000))
    x = torch.randn(B, Tn, generator=g)
    tg = torch.stack([torch.randint(0, n, (B,), generator=g) for n in widths])
    if B >= 2:
        tg[:, 0] = 0
        tg[:, 1] = torch.tensor(widths) - 1
    if regime == "amp10":
        x = 10 * x
    elif regime == "equal":
        x = torch.full((B, Tn), 0.75)
    elif regime == "dominant":
        o = 0
        for h, n in enumerate(widths):
            dom = torch.randint(0, n, (B,), generator=g)
            x[torch.arange(B), o + dom] += 250.0 * T + 12.0
            even = torch.arange(B) % 2 == 0
            tg[h] = torch.where(even, dom, tg[h])
            o += n
    return x.contiguous(), tg.contiguous()


def ce_apply(x, tg, widths, T, dt):
    """loss = mean_h mean_b CE(x_h * inv_t, target_h), d loss / d x; per-(h, b) terms [H, B].  fp64: inv_t = 1 / f32(T);
    fp32: fl(1 / T) as the kernel is handed it."""
    inv_t = torch.tensor(1.0 / f32(T), dtype=F64).to(dt)
    X = x.to(dt).clone().requires_grad_(True)
    terms = []
    o = 0
    for h, n in enumerate(widths):
        z = X[:, o:o + n] * inv_t
        terms.append(torch.logsumexp(z, 1) - z[torch.arange(x.shape[0]), tg[h]])
        o += n
    terms = torch.stack(terms)
    loss = terms.mean()
    loss.backward()
    return float(loss.detach()), X.grad, terms.detach()


def ce_grad_scale(B, H, T):
    """k / T = 1 / (B H f32(T)): dlogits is (softmax - onehot) times it."""
    return 1.0 / (B * H * f32(T))


def ce_dlogits_unit(B, H, T):
    """UNIT_DLOGITS is test_mlc.py's figure at B * H = 192, T = 0.7; dlogits is (softmax - onehot) * k / T with
    k = 1 / (B H), so the same relative accuracy of the softmax is 1e-7 * (192 * 0.7) * k / T here, never below 1e-7's own
    shape and never above one part in 1.3e-5 of a probability."""
    return UNIT_DLOGITS * max(1.0, 192.0 * f32(0.7) / (B * H * f32(T)))


# ------------------------------------------------------------------------------------------------------------------------
# k-means
# ------------------------------------------------------------------------------------------------------------------------
KM_NS = [1, 3, 4, 5, 413]
KM_DS = [1, 63, 64, 65, 512]
KM_KS = [1, 2, 8]


@functools.lru_cache(maxsize=None)
def km_case(N, D, K):
    """(emb [N, D], cent [K, D]) integer-valued fp32: embeddings in [-4, 4], centroids in [-3, 3].  Constructed ties:
    centroid K - 1 duplicates centroid 0 (K >= 2); centroid 1 is centroid 2 with coordinates 0 and 1 swapped (K >= 8, D >= 2)
    and every third embedding has equal coordinates 0 and 1, so it scores the two equally."""
    g = gen(N * 257 + D * 3 + K)
    emb = draw(g, (N, D), 4, 0.9)
    cent = draw(g, (K, D), 3, 0.9)
    if K >= 8 and D >= 2:
        cent[1] = cent[2]
        cent[1, 0], cent[1, 1] = cent[2, 1], cent[2, 0]
        emb[0::3, 1] = emb[0::3, 0]
    if K >= 2:
        cent[K - 1] = cent[0]
    return emb.float(), cent.float()


def km_ref(emb, cent):
    """fp64: assign (first maximum), counts [K], sums [K, D]."""
    sc = emb.double() @ cent.double().t()
    assign = torch.from_numpy(np.argmax(sc.numpy(), axis=1))       # numpy documents the first occurrence
    K = cent.shape[0]
    counts = torch.bincount(assign, minlength=K)
    sums = torch.zeros(K, emb.shape[1], dtype=F64).index_add_(0, assign, emb.double())
    return assign, counts, sums, sc


def km_exact(emb, cent):
    """The preconditions under which every score and every sum is exact in fp32 in any order."""
    need_exact(emb.double().abs() @ cent.double().abs().t(), quantum(emb, cent), "k-means scores")
    need_exact(emb.double().abs().sum(0), quantum(emb), "k-means sums")


def km_update_ref(cent, sums, counts):
    c = counts.double().unsqueeze(1)
    v = torch.where(c > 0, sums.double() / c.clamp_min(1), cent.double())
    return v / v.norm(dim=1, keepdim=True).clamp_min(1e-12)


# ------------------------------------------------------------------------------------------------------------------------
# derived bounds: 8 x the worst torch-fp32 restatement error over the regime's cases (never below DERIVED_FLOOR)
# ------------------------------------------------------------------------------------------------------------------------
def _att_pairs(regime):
    for (S, D, nhead) in ATT_CASES:
        for B in ATT_BS:
            qkv, dout = att_case(S, D, nhead, B, regime)
            for p in PS:
                m = bernoulli_mask((B, nhead, S, S), p, S * D + B)
                r, s = att_apply(qkv, dout, nhead, m, p, F64), att_apply(qkv, dout, nhead, m, p, F32)
                yield "out", s[0], r[0], None
                yield "dqkv", s[1], r[1], None


def ln_grad_scale(r, gamma, dout):
    """[rows, 1]: rstd * max_d |dout * gamma| of each row, the size of the terms of da = rstd (g - mean(g) - xhat mean(g xhat))
    before they cancel (with D = 1 or 2 they cancel entirely, and the result's own size says nothing about its accuracy)."""
    return r["rstd"].double().unsqueeze(1) * (dout.double() * gamma.double()).abs().max(1, keepdim=True).values


def _ln_pairs(key):
    regime, D = key
    for rows in LN_ROWS:
        a, b, gamma, beta, dout = ln_case(rows, D, regime)
        for p in PS:
            m = bernoulli_mask((rows, D), p, rows * D)
            r, s = ln_apply(a, b, gamma, beta, dout, m, p, F64), ln_apply(a, b, gamma, beta, dout, m, p, F32)
            sc = ln_grad_scale(r, gamma, dout)
            for k in ("out", "rstd", "dgamma", "dbeta"):
                yield k, s[k], r[k], None
            yield "mean", s["mean"], r["mean"], r["xabs"]
            yield "da", s["da"], r["da"], sc
            yield "db", s["db"], r["db"], sc * scale64(p)


def _head_pairs(_):
    for (S, D, Tn, l2, hb) in HEAD_CASES:
        x, W, bias, tok, gl = head_case(S, D, Tn, l2)
        b = bias if hb else None
        r, s = head_apply(x, W, b, tok, gl, l2, F64), head_apply(x, W, b, tok, gl, l2, F32)
        z = head_zero_rows(x, l2)
        sc = head_dx_scale(x, W, tok, gl, l2)
        lsc, wsc = head_out_scales(x, W, b, tok, gl, l2)
        yield "logits", s[0], r[0], lsc
        yield "dx", s[1][~z], r[1][~z], sc[~z]
        if bool(z.any()):
            yield "dx0", s[1][z], r[1][z], sc[z]
        yield "dW", s[2], r[2], wsc
        if hb:
            yield "dbias", s[3], r[3], None


def head_dx_scale(x, W, tok, gl, l2):
    """[B, S, 1]: (1 / max(|x|, 1e-12) when l2) * sum over the token's prototypes of |dlogits| max_d |W|: the size of the terms
    of dx before the projection off x cancels them (with D = 1 it cancels them entirely)."""
    B, S, _ = x.shape
    w = gl.double().abs() * W.double().abs().max(1).values              # [B, Tn]
    v = torch.zeros(B, S, dtype=F64).index_add_(1, tok.long(), w)
    if l2:
        v = v / x.double().norm(dim=2).clamp_min(1e-12)
    return v.unsqueeze(2)


def head_out_scales(x, W, bias, tok, gl, l2):
    """The sizes of what entered the logits [B, Tn] (sum_d |xn W| + |bias|) and dW [Tn, D] (sum_b |dlogits xn|): rows of x
    differ by six orders of magnitude, and an error is held against the terms of its own sum."""
    xn = x.double()
    if l2:
        xn = xn / xn.norm(dim=2, keepdim=True).clamp_min(1e-12)
    xt = xn[:, tok.long()].abs()                                            # [B, Tn, D]
    lsc = (xt * W.double().abs()).sum(2) + (0 if bias is None else bias.double().abs())
    wsc = (gl.double().abs().unsqueeze(2) * xt).sum(0)
    return lsc, wsc


def head_zero_rows(x, l2):
    """[B, S] bool: the all-zero rows under l2 (their dx is v / 1e-12, checked apart from the other rows)."""
    return (x == 0).all(2) if l2 else torch.zeros(x.shape[:2], dtype=torch.bool)


def _ce_pairs(key):
    regime, T = key
    for widths, B in CE_SHAPES:
        x, tg = ce_case(widths, B, regime, T)
        r, s = ce_apply(x, tg, widths, T, F64), ce_apply(x, tg, widths, T, F32)
        yield "loss", torch.tensor([s[0]], dtype=F64), torch.tensor([r[0]], dtype=F64), None
        yield "dlogits", s[1], r[1], ce_grad_scale(B, len(widths), T)


_FAMILIES = {"att": _att_pairs, "ln": _ln_pairs, "head": _head_pairs, "ce": _ce_pairs}


@functools.lru_cache(maxsize=None)
def restated(family, regime):
    """{quantity: worst rel_err (abs_err / max(1, |ref|) for the loss) of the fp32 restatement over the regime's cases}"""
    worst = {}
    for q, got, ref, scale in _FAMILIES[family](regime):
        worst[q] = max(worst.get(q, 0.0), measure(q, got, ref, scale))
    return worst


def measure(quantity, got, ref, scale=None):
    """The error figure of the derived bounds: |error| / max(1, |ref|) for a loss, rel_err() for everything else."""
    if quantity == "loss":
        return abs_err(got, ref) / max(1.0, float(ref.double().abs().max()))
    return rel_err(got, ref, scale)


def derived(family, regime, quantity):
    return max(DERIVED_FACTOR * restated(family, regime)[quantity], DERIVED_FLOOR)


def derived_cap(family, regime, quantity):
    """What a derived bound may be at most, from the formats alone; test_head_refs_cpu.py holds every derived bound below it, so a
    restatement that went wrong cannot loosen a GPU bound unnoticed.
      attention: 1e-4 (8 x the 1e-5 that fp32 reaches at |score| up to 190);  heads: 1e-5;  LayerNorm, unit and constant: 1e-5;
      LayerNorm, offset rows: x = a + b is rounded at 1e3 (half an ulp: 3.1e-5) before a standard deviation of 0.1 is taken out,
        3.1e-4 of xhat, times 8 and a margin of 4 for the sums over it: 1e-2; with D = 2 the two elements can be 1e-2 apart
        instead of 0.1: 1e-1;  the mean and dbeta do not see the cancellation: 1e-5;
      cross-entropy loss: 1e-4 (8 x the 8e-6 fp32 reaches at T = 0.1, amplitude 10, against max(1, |loss|));
      cross-entropy dlogits: one rounding of the scaled logit moves a probability by 2^-24 max|x / T| of itself: 8 x that,
        with max|x / T| taken as 8 at least."""
    if family == "att":
        return 1e-4
    if family == "head":
        return 1e-5
    if family == "ln":
        reg, D = regime
        if reg != "offset" or quantity in ("mean", "dbeta"):
            return 1e-5
        return 1e-1 if D == 2 else 1e-2
    reg, T = regime
    if quantity == "loss":
        return 1e-4
    top = max(float(ce_case(w, B, reg, T)[0].abs().max()) for w, B in CE_SHAPES) / f32(T)
    return DERIVED_FACTOR * 2.0 ** -24 * max(8.0, top)


def check_derived(family, regime, quantity, got, ref, scale=None, tag=""):
    """measure() of got against ref over the derived bound (<= 1 passes); recorded."""
    return record(f"{family} {quantity} ({regime}{tag})", measure(quantity, got, ref, scale), derived(family, regime, quantity))
