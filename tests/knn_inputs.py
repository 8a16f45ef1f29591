"""Test helper of the kNN edge suite (test_knn_edges_gpu.py, test_knn_refs_cpu.py): case tables, constructed similarity
rows, the fp64 restatement of the vote (csrc/knn.hip) and of the row normalisation (normalize_rows_body, csrc/ntxent.hip),
their fp32 restatements and the bounds.  CPU only: nothing here touches the library.

The vote bound is counted, per (row, label, class) with reference vote `ref`, m neighbours of that class among the k:

    |got - ref| <= (m + 4 + max|s| / T) * 2^-24 * ref

  m            the roundings of the sequential fp32 sum (one thread adds the class's weights in rank order);
  max|s| / T   the quotient s / T is rounded once before the exponential: a relative 2^-24 of the quotient moves the weight by
               that times |s / T| of itself (the maximum is over the class's voters with a finite, nonzero weight);
  4            expf (2 ulp = 4 half-ulps would be generous) and the final rounding.
Where ref is 0 or not finite the vote must be equal.  Neighbour indices and similarities are exact.  NaN similarities are
outside the vote's contract and appear nowhere here.

The normalize bound counts the roundings of the kernel's order (normalize_rows_body: one wave per row):
    for (d = lane; d < D; d += 64) s += v * v;      n = ceil(D / 64) terms per lane: one rounding of the square (none when
                                                    the compiler fuses) and one of the add, each relative to a partial sum
                                                    of positive terms: at most 1 + n roundings on any term's path
    s = wave_sum(s);                                six butterfly adds
    inv = 1.f / fmaxf(sqrtf(s), 1e-12f);            the square root halves the relative error of s and rounds once; the
                                                    reciprocal rounds once
    zn = z * inv;                                   one more
so  |inv - ref| <= ((1 + n + 6) / 2 + 2) * 2^-24 * ref   and   |zn - ref| <= ((1 + n + 6) / 2 + 3) * 2^-24 * |ref|."""
import functools
import math

import numpy as np
import torch

from edge_inputs import f32, record  # noqa: F401  (re-exported)

F64 = torch.float64
U = 2.0 ** -24
INF = float("inf")
FLT_MAX = float(np.finfo(np.float32).max)
DENORM_MIN = 2.0 ** -149
DENORM_MAX = 2.0 ** -126 - 2.0 ** -149


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------------
# the vote: fp64 restatement, fp32 restatement, bound
# ------------------------------------------------------------------------------------------------------------------------
def offsets(classes):
    off = [0]
    for c in classes:
        off.append(off[-1] + int(c))
    return off


def vote_ref(S, N, targets, classes, k, T):
    """The reference's predict from the similarity matrix on, in fp64, on S[:, :N]: stable descending sort (ties: lower index
    first, -0 == +0), exp(s / f32(T)), per-label scatter-sum that skips classes outside [0, C_l).
    -> dict votes [B, sum C] f64, idx [B, k] int64, val [B, k] f64, m [B, sum C] int64 (neighbours that voted), smax
    [B, sum C] f64 (max |s| / T over the voters with a finite nonzero weight)"""
    S = S[:, :N].double()
    B = S.shape[0]
    Tf = f32(T)
    val, idx = torch.sort(S, dim=1, descending=True, stable=True)
    val, idx = val[:, :k].contiguous(), idx[:, :k].contiguous()
    w = torch.exp(val / Tf)
    t = targets.reshape(N, -1).long()[idx]                       # [B, k, L]
    off = offsets(classes)
    votes = torch.zeros(B, off[-1], dtype=F64)
    m = torch.zeros(B, off[-1], dtype=torch.int64)
    smax = torch.zeros(B, off[-1], dtype=F64)
    counted = torch.isfinite(w) & (w > 0)
    for l, C in enumerate(classes):
        c = t[:, :, l]
        ok = (c >= 0) & (c < C)
        col = off[l] + c.clamp(0, C - 1)
        votes.scatter_add_(1, col, torch.where(ok, w, torch.zeros_like(w)))
        m.scatter_add_(1, col, ok.long())
        smax.scatter_reduce_(1, col, torch.where(ok & counted, val.abs() / Tf, torch.zeros_like(w)), "amax")
    return dict(votes=votes, idx=idx, val=val, m=m, smax=smax, T=Tf)


def vote_f32(S, N, targets, classes, k, T, idx):
    """The kernel's arithmetic in numpy fp32 on the neighbours `idx` (selection is exact, not arithmetic): the fp32 quotient,
    its exponential, and per class the sequential sum in rank order (adding 0 for the other classes' ranks changes nothing).
    -> votes [B, sum C] f32 (torch)"""
    s = np.take_along_axis(S[:, :N].numpy().astype(np.float32), idx.numpy(), axis=1)
    with np.errstate(over="ignore", under="ignore"):
        w = np.exp(s / np.float32(T)).astype(np.float32)         # [B, k]
    t = targets.reshape(N, -1).numpy().astype(np.int64)[idx.numpy()]
    out = []
    for l, C in enumerate(classes):
        hit = t[:, :, l, None] == np.arange(C)[None, None, :]    # [B, k, C]; a class outside [0, C) hits nothing
        terms = np.where(hit, w[:, :, None], np.float32(0)).astype(np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            out.append(np.cumsum(terms, axis=1, dtype=np.float32)[:, -1])
    return torch.from_numpy(np.concatenate(out, axis=1))


def vote_ratio(got, R):
    """max over (row, label, class) of |got - ref| / bound; inf when a vote whose reference is 0 or not finite is not equal, or
    when a vote is not finite where the reference is."""
    got, ref = got.double(), R["votes"]
    exact = (ref == 0) | ~torch.isfinite(ref)
    if not torch.equal(got[exact], ref[exact]):
        return math.inf
    g, r = got[~exact], ref[~exact]
    if g.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(g).all()):
        return math.inf
    lim = (R["m"][~exact].double() + 4.0 + R["smax"][~exact]) * U * r
    return float(((g - r).abs() / lim).max())


def check_votes(tag, got, R):
    """vote_ratio over 1 (<= 1 passes), recorded."""
    return record(f"knn votes ({tag})", vote_ratio(got, R), 1.0)


# ------------------------------------------------------------------------------------------------------------------------
# the row walk: N x k x ld x alignment x kind
# ------------------------------------------------------------------------------------------------------------------------
ROW_NS = [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
ROW_KINDS = ["random", "ties", "equal", "exact", "special", "negative"]
ROW_B = 5                     # with an odd ld the five rows have all four alignments modulo 16 bytes
ROW_CLASSES = (3, 2)
# Temperatures of the tables that call sm3_knn_vote directly.  |s| <= 1 in every ordinary value, so exp(s / T) is a normal
# fp32 number at each of them.  They are powers of two, for a reason of the CPU check and not of the kernel: the rounding
# of the quotient can be as large as (|s| / T) * 2^-24 (a mantissa just above 1), which is the whole of its term in the
# bound, so on a class with one voter correct fp32 arithmetic can use (|s| / T + 2) of the (5 + |s| / T) units -- within
# the bound, but not within the half of it that test_knn_refs_cpu.py demands of the fp32 restatement on every case (at
# T = 0.07 and 0.0125 the restatement reached 0.57 and 0.65 of the bound at k = 1).  With T a power of two the quotient is
# exact, and the half is left by construction to exp and to the sum.  The quotient's rounding is exercised at the
# reference's T = 0.07 through the product path (BANK_T), against the full bound.
ROW_TS = {3: 1.0, 65: 1.0, 256: 1.0, 257: 2.0 ** -6, 1023: 2.0 ** -6}
ROW_T_DEFAULT = 2.0 ** -4
BANK_T = 0.07
MAX_K = 1024
N_SPECIAL = 16                # from this N on a `special` row holds every promised bit pattern
SPECIALS = [INF, -INF, -INF, -INF, DENORM_MAX, -DENORM_MAX, DENORM_MIN, -DENORM_MIN, FLT_MAX, -FLT_MAX]
TIE_VALUES = [0.0, -0.25, -0.5, -0.75]   # the zeros rank first: k = 1 cuts between a -0 and a +0


def row_T(N):
    return ROW_TS.get(N, ROW_T_DEFAULT)


def row_ks(N):
    """1, min(N, 7), min(N, 1024), the largest power of two that fits and the number below it (not a power of two)."""
    top = min(N, MAX_K)
    ks = {1, min(N, 7), top}
    p = 1 << (top.bit_length() - 1)
    if p >= 2:
        ks.add(p)
    if p - 1 >= 3:
        ks.add(p - 1)
    return sorted(ks)


def row_lds(N):
    return [N, N + 1, N + 3, -(-N // 4) * 4 + 4]


def tie_bounds(N, ks):
    """Up to three group boundaries (ranks at which the sorted row changes value), none of them a tested k: every tested
    k < N then cuts a tie group."""
    out = []
    for want in (N // 4, N // 2, 3 * N // 4):
        b = want
        while b < N and (b in ks or b < 2):
            b += 1
        if 2 <= b < N and b not in ks and b not in out:
            out.append(b)
    return sorted(out)


def _ties_row(g, N, ks):
    bounds = [0] + tie_bounds(N, ks) + [N]
    perm = torch.randperm(N, generator=g)
    row = torch.empty(N)
    for i in range(len(bounds) - 1):
        members = perm[bounds[i]:bounds[i + 1]].sort().values
        row[members] = TIE_VALUES[i]
        if i == 0:                      # the zeros alternate -0, +0 by index: every cut inside the group is between the two
            row[members[0::2]] = -0.0
    return row


def _special_row(g, N, b):
    if N < N_SPECIAL:                   # what fits, a different stretch of the list in every row
        return torch.tensor([SPECIALS[(3 * b + i) % len(SPECIALS)] for i in range(N)], dtype=torch.float32)
    row = torch.rand(N, generator=g) * 2 - 1
    pos = torch.randperm(N, generator=g)[:len(SPECIALS)]
    row[pos] = torch.tensor(SPECIALS, dtype=F64).float()
    return row


@functools.lru_cache(maxsize=None)
def sims(kind, N, B=ROW_B):
    """[B, N] fp32 similarities of one kind (seeded by kind and N); never written to."""
    g = gen(ROW_KINDS.index(kind) * 100003 + N)
    if kind == "random":
        return torch.rand(B, N, generator=g) * 2 - 1
    if kind == "negative":
        return -0.5 - 0.5 * torch.rand(B, N, generator=g)
    if kind == "equal":
        return torch.full((B, N), 0.375)
    if kind == "exact":
        S = torch.where(torch.rand(B, N, generator=g) < 0.5, torch.zeros(B, N), torch.full((B, N), -INF))
        S[0] = 0.0                      # one row without a -inf, one without a 0
        if B > 1:
            S[1] = -INF
        return S
    if kind == "ties":
        return torch.stack([_ties_row(g, N, row_ks(N)) for _ in range(B)])
    if kind == "special":
        return torch.stack([_special_row(g, N, b) for b in range(B)])
    raise KeyError(kind)


def pad_fill(kind):
    """What stands in the columns [N, ld): +inf, which must never be chosen; 0 under the all-negative rows, as KNNBank's
    zero-padded bank rows leave it."""
    return 0.0 if kind == "negative" else INF


def padded(S, ld, fill, lead=0):
    """S [B, N] as a contiguous [B, ld] view `lead` floats into a flat buffer, the columns past N and the floats around the
    view holding `fill`.  -> (flat buffer, view)"""
    B, N = S.shape
    buf = torch.full((lead + B * ld + 4,), fill, dtype=torch.float32)
    view = buf[lead:lead + B * ld].view(B, ld)
    view[:, :N] = S
    return buf, view


@functools.lru_cache(maxsize=None)
def row_targets(N, classes=ROW_CLASSES):
    g = gen(N * 31 + len(classes))
    return torch.stack([torch.randint(0, c, (N,), generator=g) for c in classes], dim=1).to(torch.int32)


@functools.lru_cache(maxsize=None)
def row_ref(kind, N, k):
    return vote_ref(sims(kind, N), N, row_targets(N), ROW_CLASSES, k, row_T(N))


# ------------------------------------------------------------------------------------------------------------------------
# labels at the limits: 16 labels, 256 classes, the 64-rank staging chunk, classes out of range
# ------------------------------------------------------------------------------------------------------------------------
LABEL_N, LABEL_B, LABEL_T = 300, 3, 2.0 ** -4
LABEL_KS = [1, 64, 65, 200]
LABEL_SETS = {"16x16": (16,) * 16,
              "ragged": (1, 5, 2, 16, 3, 100, 1, 7, 2, 2, 31, 9, 1, 4, 64, 8),
              "1x256": (256,)}
assert all(sum(c) <= 256 and len(c) <= 16 for c in LABEL_SETS.values()) and sum(LABEL_SETS["ragged"]) == 256


@functools.lru_cache(maxsize=None)
def label_targets(name, out_of_range=False):
    """[LABEL_N, L] int32.  out_of_range: drawn from [-1, C_l], so that -1 and C_l (one below and one past the label's
    classes; the first class of the next label, had the kernel not checked) both occur in every label."""
    classes = LABEL_SETS[name]
    g = gen(len(classes) * 7 + sum(classes) + int(out_of_range))
    cols = []
    for c in classes:
        col = torch.randint(-1, c + 1, (LABEL_N,), generator=g) if out_of_range else torch.randint(0, c, (LABEL_N,), generator=g)
        if out_of_range:
            col[0], col[1] = -1, c
        cols.append(col)
    return torch.stack(cols, dim=1).to(torch.int32)


@functools.lru_cache(maxsize=None)
def label_sims():
    return torch.rand(LABEL_B, LABEL_N, generator=gen(300)) * 2 - 1


@functools.lru_cache(maxsize=None)
def label_ref(name, k, out_of_range=False):
    return vote_ref(label_sims(), LABEL_N, label_targets(name, out_of_range), LABEL_SETS[name], k, LABEL_T)


def vote_cases():
    """Every (tag, S, N, targets, classes, k, T) the GPU suite holds to the vote bound through ops.knn_vote."""
    for N in ROW_NS:
        for kind in ROW_KINDS:
            for k in row_ks(N):
                yield f"row {kind} N{N} k{k}", sims(kind, N), N, row_targets(N), ROW_CLASSES, k, row_T(N)
    for name, classes in LABEL_SETS.items():
        for oor in (False, True):
            for k in LABEL_KS:
                yield (f"labels {name} k{k}{' oor' if oor else ''}", label_sims(), LABEL_N, label_targets(name, oor), classes, k,
                       LABEL_T)


# ------------------------------------------------------------------------------------------------------------------------
# banks for the product path
# ------------------------------------------------------------------------------------------------------------------------
BANK_NS, BANK_DS, BANK_BS = [1, 2, 3, 5, 9], [1, 31, 32, 33], [1, 3]
BANK_CLASSES = (3, 2)
PAD_NS = [5, 1001]
PAD_D = 40                                  # Dp = 64: the feature width pads too
PAD_BLOCK_BYTES = {5: 1024, 1001: 1 << 16}  # column blocks of 4 and of 256 bank rows: blocks > 1 and ld > N
PAD_B = 4


@functools.lru_cache(maxsize=None)
def tiny_bank(N, D, B):
    """(bank [N, D], query [B, D], targets [N, 2]) fp32 unit rows."""
    g = gen(N * 1009 + D * 13 + B)
    bank = torch.randn(N, D, generator=g, dtype=F64)
    q = torch.randn(B, D, generator=g, dtype=F64)
    nrm = lambda t: (t / t.norm(dim=1, keepdim=True)).float()
    return nrm(bank), nrm(q), row_targets(N, BANK_CLASSES)


@functools.lru_cache(maxsize=None)
def opposed_bank(N, D=PAD_D, B=PAD_B):
    """Bank rows around a unit vector c, queries around -c (noise of norm about 0.05): every true similarity is near -1, so a
    zero from a padded bank row would be the nearest neighbour of every query."""
    g = gen(N * 17 + D)
    c = torch.randn(D, generator=g, dtype=F64)
    c = c / c.norm()
    noise = lambda n: 0.05 * torch.randn(n, D, generator=g, dtype=F64) / math.sqrt(D)
    nrm = lambda t: (t / t.norm(dim=1, keepdim=True)).float()
    return nrm(c + noise(N)), nrm(-c + noise(B)), row_targets(N, BANK_CLASSES)


def all_below(S, bound=-0.5):
    return bool((S.double() < bound).all())


# ------------------------------------------------------------------------------------------------------------------------
# row normalisation
# ------------------------------------------------------------------------------------------------------------------------
NORM_RS, NORM_DS = [1, 3, 4, 5, 9], [1, 63, 64, 65, 130, 2048]
NORM_KINDS = ["gauss", "scaled", "onehot", "zero"]
NORM_EPS = 1e-12
FLT_MIN = 2.0 ** -126


@functools.lru_cache(maxsize=None)
def norm_case(kind, R, D):
    """[R, D] fp32.  scaled: row norms from 1e-15 to 1e15 (log-spaced, shuffled), every element within [0.5, 1] of the row's
    largest, so that every square is a normal fp32 number; onehot: one +-1 per row; zero: row R // 2 (or the only row) is
    zero among gauss rows."""
    g = gen(NORM_KINDS.index(kind) * 7919 + R * 131 + D)
    if kind == "gauss":
        return torch.randn(R, D, generator=g)
    if kind == "zero":
        z = torch.randn(R, D, generator=g)
        z[R // 2] = 0.0
        return z
    if kind == "onehot":
        z = torch.zeros(R, D)
        pos = torch.randint(0, D, (R,), generator=g)
        z[torch.arange(R), pos] = torch.where(torch.arange(R) % 2 == 0, 1.0, -1.0)
        return z
    if kind == "scaled":
        v = (0.5 + 0.5 * torch.rand(R, D, generator=g, dtype=F64)) * (torch.randint(0, 2, (R, D), generator=g) * 2 - 1)
        v = v / v.norm(dim=1, keepdim=True)
        sc = torch.logspace(-15, 15, R, dtype=F64) if R > 1 else torch.tensor([1e-15], dtype=F64)
        return (v * sc[torch.randperm(R, generator=g)].unsqueeze(1)).float()
    raise KeyError(kind)


def norm_ref(z):
    """fp64: (z / max(||z||, 1e-12), 1 / max(||z||, 1e-12)) -- F.normalize(dim=1, eps=1e-12) and its factor."""
    z = z.double()
    inv = 1.0 / z.norm(dim=1).clamp_min(NORM_EPS)
    return z * inv.unsqueeze(1), inv


def norm_units(D):
    """(roundings, in units of 2^-24 of the reference, of zn; of inv_norm) -- the count of the module's header."""
    n = -(-D // 64)
    s = 1 + n + 6
    return s / 2 + 3, s / 2 + 2


def norm_f32(z):
    """The kernel in numpy fp32: lane l sums the squares of columns l, l + 64, ... in order (square and add rounded apart),
    the xor butterfly 32, 16, .., 1 folds the 64 lanes, then sqrt, max, reciprocal, product.  -> (zn, inv) torch fp32"""
    z = z.numpy().astype(np.float32)
    R, D = z.shape
    n = -(-D // 64)
    zp = np.zeros((R, n * 64), dtype=np.float32)
    zp[:, :D] = z
    zp = zp.reshape(R, n, 64)
    s = np.zeros((R, 64), dtype=np.float32)
    for i in range(n):
        s = s + zp[:, i] * zp[:, i] if i * 64 + 64 <= D else np.where(np.arange(64) + i * 64 < D, s + zp[:, i] * zp[:, i], s)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    inv = np.float32(1) / np.maximum(np.sqrt(s[:, 0]), np.float32(NORM_EPS))
    return torch.from_numpy(z * inv[:, None]), torch.from_numpy(inv)


def norm_ratios(got_zn, got_inv, z):
    """(worst |zn - ref| / bound, worst |inv - ref| / bound); a zero of the reference must be a zero."""
    zn, inv = norm_ref(z)
    uz, ui = norm_units(z.shape[1])
    gz, gi = got_zn.double(), got_inv.double()
    if not bool(torch.isfinite(gz).all() and torch.isfinite(gi).all()) or not torch.equal(gz[zn == 0], zn[zn == 0]):
        return math.inf, math.inf
    nz = zn != 0
    rz = float(((gz - zn)[nz].abs() / (uz * U * zn[nz].abs())).max()) if bool(nz.any()) else 0.0
    return rz, float(((gi - inv).abs() / (ui * U * inv)).max())
