"""CPU: the references, bounds and case tables of the multi-label head edge suites, checked without the library.

The GPU suites (test_heads_train_edges_gpu.py, test_heads_ce_kmeans_edges_gpu.py, test_heads_infer_edges_gpu.py) hold
the kernels to bounds against fp64.  Here the same formulas run in torch fp32 on the same inputs (tests/head_inputs.py)
and must stay within a quarter of every bound, derived or taken over from the existing tests; the integer cases meet
their exactness preconditions; the mask probes decode a known mask; and the case tables hold the edges they claim."""
import math

import pytest
import torch

import head_inputs as H


# ---- restatements against the fp64 references ----------------------------------------------------------------------------
# A derived bound is 8 x its restatement's error, so "restatement <= a quarter of the bound" below can only fail on a
# non-finite restatement.  What carries content is (a) the cap: every derived bound stays below what the number formats
# allow for its regime (head_inputs.derived_cap), so a restatement that went wrong cannot loosen a GPU bound unnoticed, and
# (b) the restatement against the existing unit-scale figures, which are not derived from it.
def _inside(family, regime):
    for q, e in H.restated(family, regime).items():
        assert math.isfinite(e) and e <= H.RESTATE_SHARE * H.derived(family, regime, q), (q, e)
        assert H.derived(family, regime, q) <= H.derived_cap(family, regime, q), (family, regime, q, H.derived(family, regime, q))


@pytest.mark.parametrize("regime", H.ATT_REGIMES)
def test_attention_restatement_is_inside_a_quarter_of_its_bounds(regime):
    _inside("att", regime)
    if regime == "peaked":
        return
    for (S, D, nhead) in H.ATT_CASES:
        for B in H.ATT_BS:
            qkv, dout = H.att_case(S, D, nhead, B, regime)
            for p in H.PS:
                m = H.bernoulli_mask((B, nhead, S, S), p, S * D + B)
                r, s = H.att_apply(qkv, dout, nhead, m, p, H.F64), H.att_apply(qkv, dout, nhead, m, p, H.F32)
                assert H.abs_err(s[0], r[0]) <= H.RESTATE_SHARE * H.UNIT_OUT
                for i in range(3):
                    ref = r[1][..., i * D:(i + 1) * D]
                    if float(ref.abs().max()) > 0:
                        assert H.norm_err(s[1][..., i * D:(i + 1) * D], ref) <= H.RESTATE_SHARE * H.UNIT_GRAD_NORM


@pytest.mark.parametrize("D", H.LN_DS)
@pytest.mark.parametrize("regime", H.LN_REGIMES)
def test_add_ln_restatement_is_inside_a_quarter_of_its_bounds(regime, D):
    _inside("ln", (regime, D))
    if regime == "unit":
        for rows in H.LN_ROWS:
            a, b, gamma, beta, dout = H.ln_case(rows, D, regime)
            r, s = (H.ln_apply(a, b, gamma, beta, None, None, 0.0, dt) for dt in (H.F64, H.F32))
            assert H.abs_err(s["out"], r["out"]) <= H.RESTATE_SHARE * H.UNIT_OUT


def test_offset_rows_would_be_lost_by_a_one_pass_variance():
    a, b, *_ = H.ln_case(4, 1000, "offset")
    x = (a + b).float()
    assert abs(float(x.mean()) - 1e3) < 1.0 and 0.05 < float(x.double().std()) < 0.2
    one_pass = (x * x).mean(1) - x.mean(1) ** 2                    # E[x^2] - E[x]^2 in fp32
    assert float((one_pass - x.double().var(1, unbiased=False)).abs().max()) > 0.01    # the variance itself is 0.01


def test_heads_restatement_is_inside_a_quarter_of_its_bounds():
    _inside("head", None)


@pytest.mark.parametrize("T", H.CE_TS)
@pytest.mark.parametrize("regime", H.CE_REGIMES)
def test_ce_restatement_is_inside_a_quarter_of_its_bounds(regime, T):
    _inside("ce", (regime, T))
    if regime in ("unit", "equal") and T >= 0.7:
        for widths, B in H.CE_SHAPES:
            x, tg = H.ce_case(widths, B, regime, T)
            r, s = H.ce_apply(x, tg, widths, T, H.F64), H.ce_apply(x, tg, widths, T, H.F32)
            assert abs(s[0] - r[0]) <= H.RESTATE_SHARE * H.UNIT_LOSS
            assert H.abs_err(s[1], r[1]) <= H.RESTATE_SHARE * H.ce_dlogits_unit(B, len(widths), T)


def test_ce_reference_is_torch_cross_entropy_and_its_terms_add_up():
    widths, B, T = (5, 3, 2, 3, 3, 3, 3, 2), 32, 0.7
    x, tg = H.ce_case(widths, B, "unit", T)
    loss, grad, terms = H.ce_apply(x, tg, widths, T, H.F64)
    crit = torch.nn.CrossEntropyLoss()
    want = sum(crit(p.double() / H.f32(T), t) for p, t in zip(x.split(list(widths), 1), tg)) / len(widths)
    assert abs(loss - float(want)) < 1e-12 and abs(float(terms.mean()) - loss) < 1e-12
    assert H.ce_dlogits_unit(24, 8, 0.7) == H.UNIT_DLOGITS       # the shape the figure comes from
    assert float(grad.sum(1).abs().max()) < 1e-15


# ---- exactness preconditions of the integer cases -------------------------------------------------------------------------
def test_kmeans_cases_are_exact_and_hold_ties_that_resolve_to_the_lowest_index():
    tied_dup = tied_perm = 0
    for N in H.KM_NS:
        for D in H.KM_DS:
            for K in H.KM_KS:
                emb, cent = H.km_case(N, D, K)
                assert torch.equal(emb, emb.round()) and float(emb.abs().max()) <= 4 and torch.equal(cent, cent.round())
                H.km_exact(emb, cent)
                a, counts, sums, sc = H.km_ref(emb, cent)
                assert int(counts.sum()) == N
                top = sc.max(1, keepdim=True).values
                ties = (sc == top).sum(1) > 1
                first = (sc == top).double().argmax(1)
                assert torch.equal(a, first)                        # numpy's argmax is the first maximum
                if K >= 2:
                    assert torch.equal(cent[K - 1], cent[0]) and not bool((a == K - 1).any())
                    tied_dup += int((ties & (a == 0)).sum())
                if K >= 8 and D >= 2:
                    assert torch.equal(cent[1].sort().values, cent[2].sort().values) or D > 2
                    tied_perm += int(((sc[:, 1] == sc[:, 2]) & (a == 1)).sum())
    assert tied_dup > 100 and tied_perm > 10, (tied_dup, tied_perm)


def test_integer_sums_of_the_exact_cases_stay_below_2_to_the_24():
    for rows, N in H.BRD_CASES:
        dhd = H.draw(H.gen(rows + N), (rows, N), 8, 0.8)
        H.need_exact(3.0 + dhd.abs().sum(0), 1.0, "dbias")
    for rows in H.COLSUM_ROWS:
        for N in H.COLSUM_NS:
            g = H.gen(rows * 1000 + N)
            dy, db0 = H.draw(g, (rows, N), 8, 0.9), H.draw(g, (N,), 100, 1.0)
            H.need_exact(db0.abs() + dy.abs().sum(0), 1.0, "colsum")
    with pytest.raises(AssertionError):
        H.need_exact(torch.tensor([2.0 ** 24]), 1.0, "too large")


# ---- the mask probes decode a known mask ---------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_probes_read_back_a_known_mask(p):
    B, S, D, nhead = 3, 5, 24, 8
    m = H.bernoulli_mask((B, nhead, S, S), p, 1)
    for mag in (1.0, 37.5):
        outs = [H.att_apply(H.att_probe_qkv(B, S, D, jp, mag), None, nhead, m, p, H.F32)[0] for jp in range(S)]
        assert torch.equal(H.att_mask_from_probe(outs, nhead), m)
    for rows, D in [(5, 65), (4, 1), (5, 2), (3, 1000)]:
        m = H.bernoulli_mask((rows, D), p, rows * D)
        m[0] = True                                               # an all-kept and an all-dropped row
        m[-1] = False
        for mag in (1.0, 3.25):
            r = H.ln_apply(torch.zeros(rows, D), torch.full((rows, D), mag), torch.ones(D), torch.zeros(D), None, m, p, H.F32)
            assert torch.equal(H.ln_mask_from_probe(r["out"], torch.stack([r["mean"], r["rstd"]], 1)), m), (rows, D, mag)


def test_mask_statistics_accept_a_fair_mask_and_reject_a_biased_one():
    for p in (0.1, 0.5):
        m0, m1 = H.bernoulli_mask((102400,), p, 1), H.bernoulli_mask((102400,), p, 2)
        e, lim = H.keep_rate_ok(m0, p)
        assert e <= lim
        e, lim = H.differ_ok(m0, m1, p)
        assert e <= lim
        e, lim = H.keep_rate_ok(H.bernoulli_mask((102400,), p + 0.01, 3), p)
        assert e > lim
        e, lim = H.differ_ok(m0, m0, p)
        assert e > lim


# ---- the case tables hold the edges they claim -----------------------------------------------------------------------------
def test_attention_table():
    hd = {D // n for _, D, n in H.ATT_CASES}
    assert {1, 3, 65, 512} <= hd and any(h % 4 for h in hd)
    assert (1, 4096, 8) in H.ATT_CASES and {1, 3, 5, 7, 8} <= {S for S, _, _ in H.ATT_CASES}
    assert any(S * n == 64 for S, _, n in H.ATT_CASES)             # fills the 64-row softmax stage
    assert all(S > 1 for S, _, _ in H.ATT_MASK_CASES) and set(H.ATT_MASK_CASES) <= set(H.ATT_CASES)
    for (S, D, nhead) in H.ATT_CASES:
        for B in H.ATT_BS:
            top = {r: H.att_scores(H.att_case(S, D, nhead, B, r)[0], nhead) for r in H.ATT_REGIMES}
            assert 2.9 < float(top["unit"].abs().max()) < 3.1
            assert 30 <= float(top["peaked"].abs().max()) <= 60
            assert float(top["tied"].abs().max()) == 0
            if S > 1:   # near one-hot: in the wide heads most rows, in every case at least the row with the top score
                pr = torch.softmax(top["peaked"], -1).max(-1).values
                assert float(pr.max()) > 0.999 and (D // nhead < 64 or float(pr.median()) > 0.9)


def test_layernorm_table():
    assert {1, 2, 63, 64, 65, 1000, 1024, 1025, 4096} == set(H.LN_DS) and {1, 3, 4, 5} == set(H.LN_ROWS)
    assert set(H.LN_INFER_DS) == {d for d in H.LN_DS if d <= 1024 and d != 2}
    a, b, *_ = H.ln_case(3, 64, "const")
    assert bool((a + b == H.LN_CONST).all()) and H.f32(H.LN_CONST) == H.LN_CONST


def test_bias_relu_table():
    assert {1, 255, 257, H.BRD_BIG} <= {r * n for r, n in H.BRD_CASES} and H.BRD_BIG > 4096 * 256
    assert {1, 7, 64, 100} <= {n for _, n in H.BRD_CASES}
    y, bias, _ = H.brd_case(149797, 7)
    s = (y + bias)[:, 0::2].reshape(-1)
    for v in H.BRD_TABLE:
        hit = s == v
        if v == 0:
            hit = hit & (torch.signbit(s) == (math.copysign(1.0, v) < 0))
        assert bool(hit.any()), v
    assert H.f32(H.ULP0) == H.ULP0 and H.f32(H.ULP0 / 2) == 0.0   # the smallest subnormal: one ulp around 0


def test_heads_table():
    for D in {c[1] for c in H.HEAD_CASES}:
        assert {c[3] for c in H.HEAD_CASES if c[1] == D} == {0, 1}, D
    assert {c[1] for c in H.HEAD_CASES} == {1, 7, 8, 31, 32, 33, 512, 4096}
    assert {c[2] for c in H.HEAD_CASES} == {1, 21, 31, 32, 33, 256} and {c[0] for c in H.HEAD_CASES} == {1, 3, 8}
    assert {c[4] for c in H.HEAD_CASES} == {0, 1}
    for (S, D, Tn, l2, _) in H.HEAD_CASES:
        x, W, bias, tok, gl = H.head_case(S, D, Tn, l2)
        assert int(tok.min()) >= 0 and int(tok.max()) < S
        if S >= 3:
            assert 1 not in tok.tolist()
            if Tn >= 4:
                assert bool((tok[1:] < tok[:-1]).any()) and bool((tok[1:] > tok[:-1]).any())
        n = x.double().norm(dim=2)
        z = H.head_zero_rows(x, l2)
        assert bool(z.any()) == bool(l2 and S >= 3)
        assert float(n[~z].min()) < 2e-3 and float(n.max()) > 500 and float(n.max()) < 1100


def test_ce_table():
    bh = {len(w) * B for w, B in H.CE_SHAPES}
    assert {1, 255, 256, 257, 2000} <= bh
    assert {(5, 3, 2, 3, 3, 3, 3, 2), (1, 5, 1, 2)} <= {w for w, _ in H.CE_SHAPES}
    for widths, B in H.CE_SHAPES:
        for T in H.CE_TS:
            x, tg = H.ce_case(widths, B, "dominant", T)
            o = 0
            for h, n in enumerate(widths):
                assert int(tg[h].min()) >= 0 and int(tg[h].max()) < n
                if n > 1:
                    top2 = x[:, o:o + n].double().topk(2, 1).values
                    assert float((top2[:, 0] - top2[:, 1]).min()) >= 200 * T
                    dom = x[:, o:o + n].argmax(1)
                    assert bool((tg[h][0::2] == dom[0::2]).all())
                    if B >= 16:
                        assert bool((tg[h] != dom).any())
                o += n
            if B >= 2:
                xu, tu = H.ce_case(widths, B, "unit", T)
                assert bool((tu[:, 0] == 0).all()) and bool((tu[:, 1] == torch.tensor(widths) - 1).all())
            xe, _ = H.ce_case(widths, B, "equal", T)
            assert float(xe.max()) == float(xe.min())
    x10, _ = H.ce_case((5, 3, 2, 3, 3, 3, 3, 2), 250, "amp10", 0.01)
    assert float(x10.abs().max()) / 0.01 > 3000


def test_kmeans_and_colsum_tables():
    assert set(H.KM_NS) == {1, 3, 4, 5, 413} and set(H.KM_DS) == {1, 63, 64, 65, 512} and set(H.KM_KS) == {1, 2, 8}
    assert set(H.COLSUM_ROWS) == {1, 3, 63, 64, 65, 4097} and set(H.COLSUM_NS) == {1, 63, 64, 65, 130}
    cent = torch.tensor([[3.0, 4.0], [0.0, 0.0], [0.0, 0.0]])
    got = H.km_update_ref(cent, torch.tensor([[1.0, 1.0], [9.0, 9.0], [0.0, 0.0]]), torch.tensor([2, 0, 3]))
    want = torch.tensor([[0.5, 0.5], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float64)
    want[0] /= want[0].norm()
    assert torch.allclose(got, want) and bool(torch.isfinite(got).all())
