"""CPU: the references, generators and bounds of the kNN edge suite (tests/knn_inputs.py), checked without the library.

The GPU suite (test_knn_edges_gpu.py) holds sm3_knn_vote and sm3_normalize_rows to counted bounds against fp64.  Here the
same arithmetic runs in numpy fp32 on the same inputs and must stay within half of each bound: a bound that fp32 alone
could not meet would say nothing about the kernel.  The generators' promises (every tested k cuts a tie group, a cut
between -0 and +0, all-negative rows, the special bit patterns) are asserted, and the restatement is tied to the
reference's own predictions through tests/golden/knn_ref.npz."""
import os

import numpy as np
import pytest
import torch

import knn_inputs as K


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("N", K.ROW_NS)
def test_row_walk_vote_bound_is_met_by_an_fp32_restatement(N):
    worst = 0.0
    for kind in K.ROW_KINDS:
        for k in K.row_ks(N):
            R = K.row_ref(kind, N, k)
            got = K.vote_f32(K.sims(kind, N), N, K.row_targets(N), K.ROW_CLASSES, k, K.row_T(N), R["idx"])
            r = K.vote_ratio(got, R)
            if kind == "exact":
                assert torch.equal(got.double(), R["votes"]), (kind, N, k)
            worst = max(worst, r)
    print(f"N {N}: worst fp32 restatement / bound {worst:.3f}")
    assert worst <= 0.5, worst


@pytest.mark.parametrize("name", list(K.LABEL_SETS))
def test_label_limit_vote_bound_is_met_by_an_fp32_restatement(name):
    worst = 0.0
    for oor in (False, True):
        for k in K.LABEL_KS:
            R = K.label_ref(name, k, oor)
            got = K.vote_f32(K.label_sims(), K.LABEL_N, K.label_targets(name, oor), K.LABEL_SETS[name], k, K.LABEL_T, R["idx"])
            worst = max(worst, K.vote_ratio(got, R))
    print(f"{name}: worst fp32 restatement / bound {worst:.3f}")
    assert worst <= 0.5, worst


@pytest.mark.parametrize("T", [0.07, 0.0125])
def test_at_the_reference_temperatures_fp32_meets_the_bound_but_not_its_half(T):
    """The quotient s / T rounds here, by up to (|s| / T) * 2^-24: the whole of its term.  fp32 stays inside the bound (which
    is what the GPU suite asks of the kernel at these temperatures); on one-voter classes it does not stay inside half."""
    worst = 0.0
    for N in (5, 257, 1025):
        for k in K.row_ks(N):
            R = K.vote_ref(K.sims("random", N), N, K.row_targets(N), K.ROW_CLASSES, k, T)
            got = K.vote_f32(K.sims("random", N), N, K.row_targets(N), K.ROW_CLASSES, k, T, R["idx"])
            worst = max(worst, K.vote_ratio(got, R))
    print(f"T {T}: worst fp32 restatement / bound {worst:.3f}")
    assert worst <= 1.0, worst


def test_the_case_table_is_the_one_the_restatements_cover():
    tags = [c[0] for c in K.vote_cases()]
    assert len(tags) == len(set(tags))
    assert all(c[2] <= 1025 for c in K.vote_cases())     # none is left to the GPU alone
    want = sum(len(K.row_ks(N)) for N in K.ROW_NS) * len(K.ROW_KINDS) + len(K.LABEL_SETS) * 2 * len(K.LABEL_KS)
    assert len(tags) == want


def test_vote_ratio_sees_what_it_should():
    """One ulp on one vote stays inside the bound, a dropped neighbour does not, a wrong zero or infinity is infinite."""
    R = K.row_ref("random", 65, 64)
    good = R["votes"].float()
    assert K.vote_ratio(good, R) <= 0.5
    ulp = good.clone()
    ulp[0, 0] = torch.nextafter(ulp[0, 0], torch.tensor(K.INF))
    assert K.vote_ratio(ulp, R) <= 1.0
    less = R["votes"].clone()
    col = int(K.row_targets(65)[R["idx"][0, 0], 0])              # the class of row 0's nearest neighbour for label 0
    less[0, col] -= float(torch.exp(R["val"][0, 0] / R["T"]))
    assert R["m"][0, col] >= 1 and K.vote_ratio(less.float(), R) > 1.0
    E = K.row_ref("exact", 65, 64)
    off = E["votes"].float()
    off[1] += 1.0          # row 1 is all -inf: every vote is 0
    assert K.vote_ratio(off, E) == K.INF
    Sp = K.row_ref("special", 65, 7)
    assert bool(torch.isinf(Sp["votes"]).any())
    fin = Sp["votes"].float().clone()
    fin[torch.isinf(fin)] = K.FLT_MAX
    assert K.vote_ratio(fin, Sp) == K.INF


def test_row_ks_and_lds_are_what_the_suite_promises():
    for N in K.ROW_NS:
        ks = K.row_ks(N)
        assert {1, min(N, 7), min(N, 1024)} <= set(ks) and all(1 <= k <= min(N, 1024) for k in ks)
        pow2 = [k for k in ks if k & (k - 1) == 0 and k > 1]
        odd = [k for k in ks if k & (k - 1) and k not in (min(N, 7), min(N, 1024))]
        assert (pow2 or N < 2) and (odd or N < 4 or N == 5), (N, ks)
        lds = K.row_lds(N)
        assert lds == [N, N + 1, N + 3, (N + 3) // 4 * 4 + 4] and lds[3] % 4 == 0
        # B = 5 rows of an odd ld start at all four alignments modulo 16 bytes
        for ld in lds:
            if ld % 2:
                assert {(b * ld) % 4 for b in range(K.ROW_B)} == {0, 1, 2, 3}


@pytest.mark.parametrize("N", K.ROW_NS)
def test_ties_cut_a_tie_group_at_every_k_and_between_the_zeros(N):
    S = K.sims("ties", N)
    assert len(set(S.double().unique().tolist())) <= len(K.TIE_VALUES)
    srt, idx = torch.sort(S.double(), dim=1, descending=True, stable=True)
    cut_zero = False
    for k in K.row_ks(N):
        if k == N:
            continue
        assert bool((srt[:, k - 1] == srt[:, k]).all()), (N, k)      # in every row
        a = torch.gather(S, 1, idx[:, k - 1:k])
        b = torch.gather(S, 1, idx[:, k:k + 1])
        both_zero = (a == 0) & (b == 0)
        cut_zero |= bool((both_zero & (torch.signbit(a) != torch.signbit(b))).all())
    if N >= 2:
        assert cut_zero, N
        assert bool(torch.signbit(S[S == 0]).any()) and bool((~torch.signbit(S[S == 0])).any())


def test_equal_exact_negative_and_special_hold_what_they_promise():
    finfo = np.finfo(np.float32)
    want_bits = {np.float32(v).view(np.int32).item() for v in K.SPECIALS}
    assert len(want_bits) == 8
    assert np.float32(K.DENORM_MIN).view(np.int32) == 1 and np.float32(K.DENORM_MAX).view(np.int32) == 0x007FFFFF
    assert np.float32(K.FLT_MAX) == finfo.max
    for N in K.ROW_NS:
        assert len(K.sims("equal", N).unique()) == 1
        ex = K.sims("exact", N)
        assert bool(((ex == 0) | (ex == -K.INF)).all()) and not bool(torch.signbit(ex[ex == 0]).any())
        assert bool((ex[0] == 0).all()) and bool((ex[1] == -K.INF).all())
        neg = K.sims("negative", N).double()
        assert bool((neg >= -1).all()) and bool((neg <= -0.5).all())
        sp = K.sims("special", N)
        assert not bool(torch.isnan(sp).any())
        for b in range(K.ROW_B):
            have = set(_bits(sp[b]).tolist())
            if N >= K.N_SPECIAL:
                assert want_bits <= have, (N, b)
                assert int((sp[b] == K.INF).sum()) == 1 and int((sp[b] == -K.INF).sum()) == 3
                ordinary = sp[b][(sp[b].abs() >= 2.0 ** -126) & (sp[b].abs() < 2)]
                assert ordinary.numel() == N - len(K.SPECIALS)
            else:
                assert have <= want_bits
    for kind in K.ROW_KINDS:
        assert not bool(torch.isnan(K.sims(kind, 257)).any())


def test_out_of_range_targets_hold_minus_one_and_c():
    for name, classes in K.LABEL_SETS.items():
        t = K.label_targets(name, True)
        for l, c in enumerate(classes):
            assert int(t[:, l].min()) == -1 and int(t[:, l].max()) == c
        inr = K.label_targets(name, False)
        assert bool((inr >= 0).all()) and bool((inr < torch.tensor(classes)).all())
        # a neighbour out of range casts no vote: the counts of a row sum to the in-range neighbours of each label
        R = K.label_ref(name, 200, True)
        off = K.offsets(classes)
        tt = t.long()[R["idx"]]
        for l, c in enumerate(classes):
            ok = ((tt[:, :, l] >= 0) & (tt[:, :, l] < c)).sum(1)
            assert torch.equal(R["m"][:, off[l]:off[l + 1]].sum(1), ok) and bool((ok < 200).any())


def test_opposed_banks_are_all_below_minus_a_half():
    for N in K.PAD_NS:
        bank, q, _ = K.opposed_bank(N)
        assert K.all_below(q.double() @ bank.double().T)
        assert float((bank.double().norm(dim=1) - 1).abs().max()) < 1e-6
    assert not K.all_below(torch.tensor([[-0.6, 0.0]]))


def test_restatement_predicts_what_the_reference_predicted(golden_dir):
    g = np.load(os.path.join(golden_dir, "knn_ref.npz"))
    for name in g["cases"]:
        k, C = [int(v) for v in g[f"{name}_meta"]]
        q, bank = torch.from_numpy(g[f"{name}_query"]), torch.from_numpy(g[f"{name}_bank"])
        t = torch.from_numpy(g[f"{name}_targets"])
        S = (q.double() @ bank.double().T).float()
        T = float(g[f"{name}_temperature"])
        R = K.vote_ref(S, bank.shape[0], t, [C], k, T)
        pred = R["votes"].argsort(dim=1, descending=True, stable=True)
        assert torch.equal(pred, torch.from_numpy(g[f"{name}_pred_labels"]).long()), name
        f = K.vote_f32(S, bank.shape[0], t, [C], k, T, R["idx"])
        assert K.vote_ratio(f, R) <= 0.5, name
        assert torch.equal(f.argsort(dim=1, descending=True, stable=True), pred), name


# ------------------------------------------------------------------------------------------------------------------------
# normalize
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", K.NORM_DS)
def test_normalize_bound_is_met_by_an_fp32_restatement_in_the_kernels_order(D):
    worst = 0.0
    for R in K.NORM_RS:
        for kind in K.NORM_KINDS:
            z = K.norm_case(kind, R, D)
            zn, inv = K.norm_f32(z)
            rz, ri = K.norm_ratios(zn, inv, z)
            worst = max(worst, rz, ri)
            if kind == "onehot":
                assert torch.equal(zn, z) and bool((inv == 1).all())
            if kind == "zero":
                assert bool((zn[R // 2] == 0).all()) and float(inv[R // 2]) == float(np.float32(1e12))
    print(f"D {D}: worst fp32 restatement / bound {worst:.3f}")
    assert worst <= 0.5, worst


def test_normalize_reference_is_f_normalize_and_the_count_is_the_formula():
    for D in K.NORM_DS:
        z = K.norm_case("zero", 5, D)
        zn, inv = K.norm_ref(z)
        want = torch.nn.functional.normalize(z.double(), dim=1, eps=1e-12)
        assert float((zn - want).abs().max()) < 1e-15
        assert bool((zn[2] == 0).all()) and float(inv[2]) == 1e12
    assert K.norm_units(1) == (7.0, 6.0) and K.norm_units(64) == (7.0, 6.0)
    assert K.norm_units(65) == (7.5, 6.5) and K.norm_units(2048) == (22.5, 21.5)


def test_scaled_rows_span_thirty_decades_with_normal_squares():
    for R in K.NORM_RS:
        for D in K.NORM_DS:
            z = K.norm_case("scaled", R, D).double()
            sq = z * z
            assert float(sq.min()) >= K.FLT_MIN and float(sq.sum(1).max()) < K.FLT_MAX
            n = z.norm(dim=1)
            if R >= 3:
                assert float(n.min()) < 2e-15 and float(n.max()) > 5e14
    one = K.norm_case("onehot", 5, 65)
    assert bool(((one != 0).sum(1) == 1).all()) and bool((one.abs().sum(1) == 1).all())
