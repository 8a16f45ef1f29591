"""GPU: the weighted-kNN path at its edges -- sm3_knn_vote (csrc/knn.hip), KNNBank / knn_scores / normalize
(sm3hip/knn.py) and the forward normalize_rows_kernel (csrc/ntxent.hip) -- against the fp64 restatements of
tests/knn_inputs.py.

Neighbour indices and similarities are compared with torch.equal (ties: lower index first, -0 == +0).  Votes are held to
the counted bound (m + 4 + max|s| / T) * 2^-24 * ref per (row, label, class), and are equal where the reference is 0 or
infinite; with similarities in {0, -inf} they are integer counts and equal.  Normalised rows are held to the counted
bound of knn_inputs.norm_units().  tests/test_knn_refs_cpu.py shows numpy fp32 inside half of both bounds on the same
inputs.  Every output is a slice of a sentinel-filled buffer whose surroundings must come back unchanged, and every
similarity matrix a view into a larger buffer."""
import numpy as np
import pytest
import torch

import knn_inputs as K
from exact_inputs import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ops():
    from sm3hip import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _dev_targets(targets, spare=8):
    """[N, L] int32 on the GPU as the head of a larger zero buffer."""
    N, L = targets.shape
    buf = torch.zeros(N + spare, L, dtype=torch.int32, device=DEV)
    buf[:N] = targets.to(DEV)
    return buf[:N]


def _dev_sims(S, ld, fill, lead):
    buf, _ = K.padded(S, ld, fill, lead)
    B = S.shape[0]
    return buf.to(DEV)[lead:lead + B * ld].view(B, ld)


def _vote(Sd, N, td, classes, k, T, neighbors=True):
    """ops.knn_vote into guarded outputs -> (votes, idx, sim) on the CPU."""
    B = Sd.shape[0]
    off = K.offsets(classes)
    sc = Guarded(B * off[-1], torch.float32)
    ix = Guarded(B * k, torch.int32)
    sm = Guarded(B * k, torch.float32)
    _ops().knn_vote(Sd, N, td, off, k, T, sc.t.view(B, off[-1]), ix.t.view(B, k) if neighbors else None,
                    sm.t.view(B, k) if neighbors else None)
    torch.cuda.synchronize()
    assert sc.guards() and ix.guards() and sm.guards()
    if not neighbors:
        assert ix.untouched() and sm.untouched()
    return sc.t.view(B, off[-1]).cpu(), ix.t.view(B, k).cpu(), sm.t.view(B, k).cpu()


def _check(tag, out, R, exact=False):
    votes, idx, sim = out
    assert torch.equal(idx.long(), R["idx"]), tag
    assert torch.equal(sim.double(), R["val"]), tag
    if exact:
        assert torch.equal(votes.double(), R["votes"]), tag
    ratio = K.check_votes(tag, votes, R)
    assert ratio <= 1.0, (tag, ratio)


# ------------------------------------------------------------------------------------------------------------------------
# a. the row walk, c. (second half) the same bits at every ld and alignment
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.ROW_KINDS)
@pytest.mark.parametrize("N", K.ROW_NS)
def test_row_walk_at_every_n_k_ld_and_alignment(N, kind):
    """N from 1 to 1025 (no 16-byte group, idle threads, partial waves, the partly filled 4 x 256 unroll), every k of row_ks,
    ld in {N, N + 1, N + 3, a multiple of 4} with five rows (aligned, scalar and mixed launches), the base moved by one float."""
    S, td, T = K.sims(kind, N), _dev_targets(K.row_targets(N)), K.row_T(N)
    fill = K.pad_fill(kind)
    for k in K.row_ks(N):
        R = K.row_ref(kind, N, k)
        first = None
        for ld in K.row_lds(N):
            for lead in (0, 1):
                Sd = _dev_sims(S, ld, fill, lead)
                assert Sd.is_contiguous() and Sd.data_ptr() % 16 == 4 * lead
                out = _vote(Sd, N, td, K.ROW_CLASSES, k, T)
                if first is None:
                    first = out
                    _check(f"row {kind} T{T}", out, R, exact=(kind == "exact"))
                assert _same_bits(out, first), (N, kind, k, ld, lead)
        assert int(first[1].max()) < N


def test_without_neighbour_outputs_the_votes_are_the_same_bits():
    N, k = 257, 255
    Sd, td = _dev_sims(K.sims("random", N), N + 1, K.INF, 1), _dev_targets(K.row_targets(N))
    a = _vote(Sd, N, td, K.ROW_CLASSES, k, K.row_T(N))
    b = _vote(Sd, N, td, K.ROW_CLASSES, k, K.row_T(N), neighbors=False)
    assert torch.equal(_bits(a[0]), _bits(b[0]))


@pytest.mark.parametrize("T", [0.07, 0.0125])
@pytest.mark.parametrize("N", [5, 257, 1025])
def test_row_walk_at_the_reference_temperatures(N, T):
    """The tables above run at power-of-two temperatures (knn_inputs.ROW_TS says why); here the quotient s / T rounds, at
    the reference's default and at |s| / T up to 80, against the same bound."""
    S, td = K.sims("random", N), _dev_targets(K.row_targets(N))
    for k in K.row_ks(N):
        R = K.vote_ref(S, N, K.row_targets(N), K.ROW_CLASSES, k, T)
        _check(f"row random T{T}", _vote(_dev_sims(S, N + 1, K.INF, 0), N, td, K.ROW_CLASSES, k, T), R)


# ------------------------------------------------------------------------------------------------------------------------
# b. labels at the limits
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("oor", [False, True], ids=["in_range", "out_of_range"])
@pytest.mark.parametrize("name", list(K.LABEL_SETS))
def test_labels_at_the_limits(name, oor):
    """16 labels, 256 classes over all labels, k on either side of the 64-rank staging chunk; the L-label call equals the L
    single-label calls bit for bit; a target of -1 or C_l is a neighbour like any other and casts no vote."""
    classes, N = K.LABEL_SETS[name], K.LABEL_N
    t = K.label_targets(name, oor)
    td = _dev_targets(t)
    Sd = _dev_sims(K.label_sims(), N + 1, K.INF, 0)
    off = K.offsets(classes)
    for k in K.LABEL_KS:
        R = K.label_ref(name, k, oor)
        out = _vote(Sd, N, td, classes, k, K.LABEL_T)
        _check(f"labels {name}{' out of range' if oor else ''}", out, R)
        if oor:
            tt = t.long()[out[1].long()]                                    # [B, k, L]
            bad = (tt < 0) | (tt >= torch.tensor(classes))
            assert bool(bad.any()) or k == 1
            assert torch.equal(R["m"].sum(1), (~bad).sum((1, 2)))
        for l, c in enumerate(classes):
            single = _vote(Sd, N, _dev_targets(t[:, l:l + 1].contiguous()), [c], k, K.LABEL_T)
            assert torch.equal(_bits(single[0]), _bits(out[0][:, off[l]:off[l + 1]])), (name, k, l)
            assert _same_bits(single[1:], out[1:])


# ------------------------------------------------------------------------------------------------------------------------
# c. bits do not depend on placement
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "ties", "special"])
@pytest.mark.parametrize("N", [5, 65, 257, 1025])
def test_a_row_gives_the_same_bits_alone_first_last_and_again(N, kind):
    S5 = K.sims(kind, N)
    row = S5[2:3]
    big = K.sims("random", N, 37).clone()
    big[0], big[36] = row[0], row[0]
    td = _dev_targets(K.row_targets(N))
    k, T = K.row_ks(N)[-2] if N > 1 else 1, K.row_T(N)
    alone = _vote(_dev_sims(row, N + 3, K.INF, 0), N, td, K.ROW_CLASSES, k, T)
    _check(f"row {kind} T{T}", alone, {key: (v[2:3] if torch.is_tensor(v) else v) for key, v in K.row_ref(kind, N, k).items()})
    Bd = _dev_sims(big, N + 1, K.INF, 1)      # rows 0 and 36 start at different alignments
    many = _vote(Bd, N, td, K.ROW_CLASSES, k, T)
    again = _vote(Bd, N, td, K.ROW_CLASSES, k, T)
    assert _same_bits(many, again)
    for pos in (0, 36):
        assert _same_bits([o[pos:pos + 1] for o in many], alone), (N, kind, pos)


# ------------------------------------------------------------------------------------------------------------------------
# d. through KNNBank / knn_scores
# ------------------------------------------------------------------------------------------------------------------------
def _scores_and_s(q, bank, k, T):
    from sm3hip.knn import knn_scores
    votes, (idx, sim) = knn_scores(q, bank, k=k, temperature=T, neighbors=True)
    qp = torch.nn.functional.pad(q, (0, bank.Dp - bank.D))
    Sg = Guarded(q.shape[0] * bank.ld, torch.float32)
    S = Sg.t.view(q.shape[0], bank.ld)
    bank.similarity(qp, S)
    torch.cuda.synchronize()
    assert Sg.guards()
    return torch.cat(votes, dim=1).cpu(), idx.cpu(), sim.cpu(), S.cpu()


@pytest.mark.parametrize("B", K.BANK_BS)
@pytest.mark.parametrize("D", K.BANK_DS)
@pytest.mark.parametrize("N", K.BANK_NS)
def test_tiny_banks_through_the_product(N, D, B):
    """Banks of 1 to 9 rows (Nc = 4, 8 or 12), D in {1, 31, 32, 33} (Dp = 32 or 64), one query or three: S against fp64, the
    votes against the restatement on the same S."""
    from sm3hip.knn import KNNBank
    bank_f, q, t = K.tiny_bank(N, D, B)
    bank = KNNBank(bank_f.to(DEV), t.to(DEV), list(K.BANK_CLASSES))
    assert bank.ld % 4 == 0 and bank.ld >= N and bank.Dp % 32 == 0
    S64 = q.double() @ bank_f.double().T
    for k in sorted({1, N}):
        votes, idx, sim, S = _scores_and_s(q.to(DEV), bank, k, K.BANK_T)
        assert float((S[:, :N].double() - S64).abs().max()) < 1e-5
        assert bool((S[:, N:] == 0).all())
        _check("bank tiny", (votes, idx, sim), K.vote_ref(S, N, t, K.BANK_CLASSES, k, K.BANK_T))


@pytest.mark.parametrize("blocked", [False, True], ids=["one_block", "column_blocks"])
@pytest.mark.parametrize("N", K.PAD_NS)
def test_padding_columns_cannot_win(N, blocked):
    """Every true similarity is below -0.5 and S[:, N:ld] is 0: a kernel that read ld columns would rank a padding column
    first for every query."""
    from sm3hip.knn import KNNBank
    bank_f, q, t = K.opposed_bank(N)
    assert K.all_below(q.double() @ bank_f.double().T)
    kw = dict(block_bytes=K.PAD_BLOCK_BYTES[N]) if blocked else {}
    bank = KNNBank(bank_f.to(DEV), t.to(DEV), list(K.BANK_CLASSES), **kw)
    assert bank.ld > N and (bank.blocks > 1) == blocked
    for k in sorted({1, min(N, 200)}):
        votes, idx, sim, S = _scores_and_s(q.to(DEV), bank, k, K.BANK_T)
        assert bool((S[:, N:] == 0).all()) and K.all_below(S[:, :N])
        assert int(idx.max()) < N and int(idx.min()) >= 0 and K.all_below(sim)
        _check("bank opposed", (votes, idx, sim), K.vote_ref(S, N, t, K.BANK_CLASSES, k, K.BANK_T))


# ------------------------------------------------------------------------------------------------------------------------
# e. knn.normalize
# ------------------------------------------------------------------------------------------------------------------------
def _normalize(z):
    """ops.normalize_rows into guarded outputs, and knn.normalize, which must agree -> (zn, inv) on the CPU."""
    from sm3hip.knn import normalize
    R, D = z.shape
    zd = z.to(DEV)
    zn, inv = Guarded(R * D, torch.float32), Guarded(R, torch.float32)
    _ops().normalize_rows(zd, zn.t.view(R, D), inv.t)
    torch.cuda.synchronize()
    assert zn.guards() and inv.guards()
    assert torch.equal(_bits(normalize(zd)), _bits(zn.t.view(R, D)))
    return zn.t.view(R, D).cpu(), inv.t.cpu()


@pytest.mark.parametrize("kind", K.NORM_KINDS)
@pytest.mark.parametrize("D", K.NORM_DS)
@pytest.mark.parametrize("R", K.NORM_RS)
def test_normalize_against_fp64(R, D, kind):
    z = K.norm_case(kind, R, D)
    zn, inv = _normalize(z)
    rz, ri = K.norm_ratios(zn, inv, z)
    K.record(f"normalize zn ({kind})", rz, 1.0)
    K.record(f"normalize inv_norm ({kind})", ri, 1.0)
    assert rz <= 1.0 and ri <= 1.0, (R, D, kind, rz, ri)
    if kind == "onehot":
        assert torch.equal(zn, z) and bool((inv == 1).all())
    if kind == "zero":
        assert bool((zn[R // 2] == 0).all()) and float(inv[R // 2]) == float(np.float32(1e12))


@pytest.mark.parametrize("D", K.NORM_DS)
def test_a_normalized_row_does_not_depend_on_its_place(D):
    src = K.norm_case("scaled", 9, D)
    row = src[4:5]
    alone = _normalize(row)
    for R, pos in ((9, 0), (9, 3), (9, 4), (9, 8), (5, 4)):
        z = K.norm_case("gauss", R, D).clone()
        z[pos] = row[0]
        zn, inv = _normalize(z)
        assert torch.equal(_bits(zn[pos:pos + 1]), _bits(alone[0])) and torch.equal(_bits(inv[pos:pos + 1]), _bits(alone[1]))
