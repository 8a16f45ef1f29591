"""GPU: the training kernels of the multi-label heads (csrc/heads_train.hip) at their edges, called through the C ABI:
attention forward / backward in both row layouts, add-LayerNorm forward and both backward forms, bias-ReLU-dropout and
its backward, the atomic column sum, the prototype heads forward and both backward forms.

Dropout masks are read from the forward kernels with operands that reduce the answer to "zero or not" (head_inputs.py);
forward and backward are then held to an fp64 autograd reference that uses the probed mask.  Every output is a Guarded
slice whose guard bytes must survive the launch; a refused call must leave the whole buffer untouched.  Bounds:
head_inputs.py (exact where a result is one fp32 operation, a copy or an integer sum; the project's unit-scale figures;
8 x the torch-fp32 restatement's error elsewhere)."""
import ctypes as C
import functools

import pytest
import torch

import head_inputs as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


def _lib():
    from sm3hip import _lib as L
    return L.load()


def _P(t):
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p((t.t if isinstance(t, H.Guarded) else t).data_ptr())


def _g(n, fill=None):
    return H.Guarded(int(n), F32, fill)


_KEEP = []


def _dev(t):
    """An input on the GPU, kept alive until _done(): only its address is handed to the launch."""
    _KEEP.append(t.contiguous().to(DEV))
    return _KEEP[-1]


def _done(*bufs):
    torch.cuda.synchronize()
    _KEEP.clear()
    assert all(b.guards() for b in bufs), "a launch wrote outside its output"


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------
def _att_fwd(qkv, nhead, p, seed, lm):
    """qkv logical [B, S, 3D] (CPU) -> out logical [B, S, D] (CPU)"""
    B, S, D3 = qkv.shape
    D = D3 // 3
    rows = _dev(H.to_rows(qkv, lm))
    o = _g(B * S * D)
    assert _lib().sm3_mlc_attention_fwd(_P(rows), _P(o), B, S, D, nhead, p, seed, lm, None) == 0
    _done(o)
    return H.from_rows(o.t.cpu().view(B * S, D), B, S, lm)


def _att_bwd(qkv, dout, nhead, p, seed, lm):
    B, S, D3 = qkv.shape
    D = D3 // 3
    o = _g(B * S * D3)
    assert _lib().sm3_mlc_attention_bwd(_P(_dev(H.to_rows(qkv, lm))), _P(_dev(H.to_rows(dout, lm))), _P(o), B, S, D, nhead, p,
                                        seed, lm, None) == 0
    _done(o)
    return H.from_rows(o.t.cpu().view(B * S, D3), B, S, lm)


@functools.lru_cache(maxsize=None)
def _att_mask(B, S, D, nhead, p, seed, lm, mag=1.0):
    """[B, nhead, S, S] bool, read from S forward launches (never written to afterwards)."""
    return H.att_mask_from_probe([_att_fwd(H.att_probe_qkv(B, S, D, jp, mag), nhead, p, seed, lm) for jp in range(S)], nhead)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("S,D,nhead", H.ATT_MASK_CASES, ids=str)
def test_attention_mask_depends_on_seed_and_index_only(S, D, nhead, p):
    B = 3
    m = _att_mask(B, S, D, nhead, p, 11, 1)
    assert torch.equal(m, _att_mask(B, S, D, nhead, p, 11, 0)), "the mask differs between the row layouts"
    assert torch.equal(m, _att_mask(B, S, D, nhead, p, 11, 1, 37.5)), "the mask depends on the operands"
    assert torch.equal(m[:1], _att_mask(1, S, D, nhead, p, 11, 1)), "the mask of sample 0 depends on B"
    if (S, D, nhead) == (8, 64, 8):   # 64 bits per (b, h): a dropped index term would make these copies
        assert not bool((m == m[:1]).all()), "every sample has the mask of sample 0"
        assert not bool((m == m[:, :1]).all()), "every head has the mask of head 0"
        assert not bool((m == m[:, :, :1]).all()), "every query row has the mask of row 0"
        assert not bool((m == m[..., :1]).all()), "every key has the mask of key 0"


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_keep_rate_and_seeds(p):
    """B = 200 for this test alone: 200 * 8 * 8 * 8 = 102400 mask elements (hd = 1, eight tiny launches per mask)."""
    m0, m1 = _att_mask(200, 8, 8, 8, p, 5, 1), _att_mask(200, 8, 8, 8, p, 6, 1)
    assert m0.numel() >= 100000
    for m in (m0, m1):
        err, lim = H.keep_rate_ok(m, p)
        assert H.record(f"attention keep rate (p {p})", err, lim) <= 1.0
    err, lim = H.differ_ok(m0, m1, p)
    assert H.record(f"attention masks of two seeds (p {p})", err, lim) <= 1.0


@pytest.mark.parametrize("B", H.ATT_BS)
@pytest.mark.parametrize("S,D,nhead", H.ATT_CASES, ids=str)
def test_attention_forward_and_backward_against_fp64(S, D, nhead, B):
    for p in H.PS:
        mask = _att_mask(B, S, D, nhead, p, 23, 1) if p > 0 else None
        for regime in H.ATT_REGIMES:
            qkv, dout = H.att_case(S, D, nhead, B, regime)
            ref_out, ref_d = H.att_apply(qkv, dout, nhead, mask, p, H.F64)
            out, dq = _att_fwd(qkv, nhead, p, 23, 1), _att_bwd(qkv, dout, nhead, p, 23, 1)
            assert _bits(out, _att_fwd(qkv, nhead, p, 23, 0)), ("forward bits differ between the layouts", regime, p)
            assert _bits(dq, _att_bwd(qkv, dout, nhead, p, 23, 0)), ("backward bits differ between the layouts", regime, p)
            what = (S, D, nhead, B, regime, p)
            assert H.check_derived("att", regime, "out", out, ref_out) <= 1.0, what
            assert H.check_derived("att", regime, "dqkv", dq, ref_d) <= 1.0, what
            if regime != "peaked":
                assert H.record(f"attention out, existing figure ({regime})", H.abs_err(out, ref_out), H.UNIT_OUT) <= 1.0, what
                for i, nm in enumerate("qkv"):
                    r = ref_d[..., i * D:(i + 1) * D]
                    if float(r.abs().max()) > 0:
                        e = H.norm_err(dq[..., i * D:(i + 1) * D], r)
                        assert H.record(f"attention d{nm}, norm-wise ({regime})", e, H.UNIT_GRAD_NORM) <= 1.0, what
            if S == 1 and p == 0:   # the softmax over one candidate is 1 by definition
                H.same(out.to(DEV), qkv[..., 2 * D:], "S = 1: out is V")
                H.same(dq[..., 2 * D:].to(DEV), dout, "S = 1: dV is dO")
                H.same(dq[..., :2 * D].to(DEV), torch.zeros(B, S, 2 * D), "S = 1: dQ and dK are zero")


# ------------------------------------------------------------------------------------------------------------------------
# add-LayerNorm
# ------------------------------------------------------------------------------------------------------------------------
def _ln_fwd(a, b, gamma, beta, p, seed):
    rows, D = a.shape
    out, st = _g(rows * D), _g(rows * 2)
    assert _lib().sm3_mlc_add_ln_fwd(_P(_dev(a)), _P(_dev(b)), _P(_dev(gamma)), _P(_dev(beta)), H.EPS, p, seed, _P(out), _P(st),
                                     rows, D, None) == 0
    _done(out, st)
    return out.t.cpu().view(rows, D), st.t.cpu().view(rows, 2)


def _ln_mask(rows, D, p, seed, mag=1.0):
    out, st = _ln_fwd(torch.zeros(rows, D), torch.full((rows, D), mag), torch.ones(D), torch.zeros(D), p, seed)
    return H.ln_mask_from_probe(out, st)


DG0, DB0 = 0.5, -0.25   # dgamma / dbeta start here: the kernels accumulate


def _ln_bwd(dout, a, b, st, gamma, p, seed, det):
    rows, D = a.shape
    da, db = _g(rows * D), _g(rows * D)
    dg, dbe = _g(D, torch.full((D,), DG0)), _g(D, torch.full((D,), DB0))
    args = [_P(_dev(dout)), _P(_dev(a)), _P(_dev(b)), _P(_dev(st)), _P(_dev(gamma)), p, seed, _P(da), _P(db), _P(dg), _P(dbe)]
    if det:
        assert _lib().sm3_mlc_add_ln_bwd_det(*args, None, rows, D, None) == 0     # rows <= 256: one slab, no workspace
    else:
        assert _lib().sm3_mlc_add_ln_bwd(*args, rows, D, None) == 0
    _done(da, db, dg, dbe)
    return da.t.cpu().view(rows, D), db.t.cpu().view(rows, D), dg.t.cpu() - DG0, dbe.t.cpu() - DB0, dg.t.cpu()


@pytest.mark.parametrize("rows", H.LN_ROWS)
@pytest.mark.parametrize("D", H.LN_DS)
def test_add_ln_forward_and_both_backward_forms_against_fp64(D, rows):
    for p in H.PS:
        mask = _ln_mask(rows, D, p, 31) if p > 0 else None
        for regime in H.LN_REGIMES:
            a, b, gamma, beta, dout = H.ln_case(rows, D, regime)
            ref = H.ln_apply(a, b, gamma, beta, dout, mask, p, H.F64)
            out, st = _ln_fwd(a, b, gamma, beta, p, 31)
            key, what = (regime, D), (D, rows, regime, p)
            assert H.check_derived("ln", key, "out", out, ref["out"]) <= 1.0, what
            assert H.check_derived("ln", key, "mean", st[:, 0], ref["mean"], ref["xabs"]) <= 1.0, what
            assert H.check_derived("ln", key, "rstd", st[:, 1], ref["rstd"]) <= 1.0, what
            if regime == "unit":
                assert H.record("add_ln out, existing figure (unit)", H.abs_err(out, ref["out"]), H.UNIT_OUT) <= 1.0, what
            sc = H.ln_grad_scale(ref, gamma, dout)
            forms = [_ln_bwd(dout, a, b, st, gamma, p, 31, det) for det in (False, True)]
            for (da, db, dg, dbe, _), form in zip(forms, ("atomic", "det")):
                assert H.check_derived("ln", key, "da", da, ref["da"], sc) <= 1.0, (what, form)
                assert H.check_derived("ln", key, "db", db, ref["db"], sc * H.scale64(p)) <= 1.0, (what, form)
                # DG0 / DB0 were added in fp32 and subtracted again: one rounding of the sum each way
                assert H.check_derived("ln", key, "dgamma", dg, ref["dgamma"], ref["dgamma"].abs().max() + DG0,
                                       tag=", " + form) <= 1.0, (what, form)
                assert H.check_derived("ln", key, "dbeta", dbe, ref["dbeta"], ref["dbeta"].abs().max() + abs(DB0),
                                       tag=", " + form) <= 1.0, (what, form)
            assert _bits(forms[0][0], forms[1][0]) and _bits(forms[0][1], forms[1][1]), ("da / db differ between the forms", what)
            if regime == "const" and p == 0 and (D & (D - 1)) == 0:
                # D copies of 1.5 sum exactly: mean = 1.5, xhat = 0, out = beta, and dgamma receives exact zeros
                H.same(out.to(DEV), beta.expand(rows, D), "constant row: out is beta")
                H.same(st[:, 0].to(DEV), torch.full((rows,), H.LN_CONST), "constant row: mean")
                for f in forms:
                    H.same(f[4].to(DEV), torch.full((D,), DG0), "constant row: dgamma unchanged")


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_add_ln_mask_depends_on_seed_and_index_only(p):
    rows, D = 25, 4096                                   # 102400 elements
    m0, m1 = _ln_mask(rows, D, p, 7), _ln_mask(rows, D, p, 8)
    assert torch.equal(m0, _ln_mask(rows, D, p, 7, 3.25)), "the mask depends on the operands"
    assert torch.equal(m0[:5], _ln_mask(5, D, p, 7)), "the mask of a row depends on the row count"
    assert not bool((m0 == m0[:1]).all()), "every row has the mask of row 0"
    for m in (m0, m1):
        err, lim = H.keep_rate_ok(m, p)
        assert H.record(f"add_ln keep rate (p {p})", err, lim) <= 1.0
    err, lim = H.differ_ok(m0, m1, p)
    assert H.record(f"add_ln masks of two seeds (p {p})", err, lim) <= 1.0
    # the narrow register form (D <= 1024) reads the same stream: element row * D + d of stream `seed`
    assert torch.equal(_ln_mask(5, 1000, p, 7).reshape(-1)[:4096], m0[0]), "the two register forms index the stream differently"


# ------------------------------------------------------------------------------------------------------------------------
# bias-ReLU-dropout, colsum
# ------------------------------------------------------------------------------------------------------------------------
def _brd_fwd(y, bias, p, seed):
    rows, N = y.shape
    h, hd = _g(rows * N), _g(rows * N)
    assert _lib().sm3_mlc_bias_relu_drop_fwd(_P(_dev(y)), _P(_dev(bias)), p, seed, _P(h), _P(hd), rows, N, None) == 0
    _done(h, hd)
    return h.t.view(rows, N), hd.t.view(rows, N)


def _brd_mask(rows, N, p, seed, mag=1.0):
    return _brd_fwd(torch.full((rows, N), mag), torch.zeros(N), p, seed)[1] != 0


def _brd_bwd(dhd, h, p, seed, dbias0):
    rows, N = h.shape
    dh = _g(rows * N)
    dbias = None if dbias0 is None else _g(N, dbias0)
    assert _lib().sm3_mlc_relu_drop_bwd(_P(_dev(dhd)), _P(h), p, seed, _P(dh), _P(dbias), rows, N, None) == 0
    _done(*([dh] if dbias is None else [dh, dbias]))
    return dh.t.view(rows, N), None if dbias is None else dbias.t


def _sum_limit(terms_abs, n):
    """A sum of n fp32 terms in any order is within (n - 1) 2^-24 sum|terms| of the exact one (first order), plus the
    rounding of the stored result."""
    return (max(n - 1, 0) + 1) * 2.0 ** -24 * terms_abs + 2.0 ** -149


@pytest.mark.parametrize("p", H.PS)
@pytest.mark.parametrize("rows,N", H.BRD_CASES, ids=str)
def test_bias_relu_dropout_is_exact(rows, N, p):
    y, bias, dhd = H.brd_case(rows, N)
    mask = _brd_mask(rows, N, p, 41).cpu() if p > 0 else torch.ones(rows, N, dtype=torch.bool)
    if p > 0:
        assert torch.equal(mask, _brd_mask(rows, N, p, 41, 2.5e-3).cpu()), "the mask depends on the operands"
    scale = torch.tensor(H.scale32(p), dtype=F32)
    h, hd = _brd_fwd(y, bias, p, 41)
    h_ref = torch.relu(y + bias)                                        # the references: single fp32 operations on the CPU
    H.same(h, h_ref, "h = relu(y + bias)")
    hd_ref = torch.where(mask, h_ref * scale, torch.zeros(()))
    H.same(hd, hd_ref, "hd = h * scale where kept")
    dh, dbias = _brd_bwd(dhd, h, p, 41, torch.full((N,), 0.5))
    dh_ref = torch.where(mask & (h_ref > 0), dhd * scale, torch.zeros(()))
    H.same(dh, dh_ref, "dh = dhd * scale where kept and h > 0")
    ref = 0.5 + dh_ref.double().sum(0)
    lim = _sum_limit(0.5 + dh_ref.double().abs().sum(0), rows + 1)
    assert H.record("relu_drop_bwd dbias", float(((dbias.cpu().double() - ref).abs() / lim).max()), 1.0) <= 1.0
    dh2, _ = _brd_bwd(dhd, h, p, 41, None)                              # dbias null: dh alone
    assert _bits(dh, dh2)


@pytest.mark.parametrize("rows,N", H.BRD_CASES, ids=str)
def test_relu_drop_bwd_dbias_on_integers_is_exact(rows, N):
    y, bias, _ = H.brd_case(rows, N)
    dhd = H.draw(H.gen(rows + N), (rows, N), 8, 0.8)
    H.need_exact(3.0 + dhd.abs().sum(0), 1.0, "dbias")
    h, _ = _brd_fwd(y, bias, 0.0, 1)
    dh, dbias = _brd_bwd(dhd.float(), h, 0.0, 1, torch.full((N,), 3.0))
    ref = 3.0 + (dhd * (torch.relu(y + bias) > 0)).sum(0)
    H.same(dbias, ref, "dbias on integers")


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_bias_relu_dropout_keep_rate_and_seeds(p):
    rows, N = 149797, 7                                                  # 4096 * 256 + 3 elements: the second grid sweep
    m0, m1 = _brd_mask(rows, N, p, 3), _brd_mask(rows, N, p, 4)
    for m in (m0, m1):
        err, lim = H.keep_rate_ok(m.cpu(), p)
        assert H.record(f"bias_relu_drop keep rate (p {p})", err, lim) <= 1.0
    err, lim = H.differ_ok(m0.cpu(), m1.cpu(), p)
    assert H.record(f"bias_relu_drop masks of two seeds (p {p})", err, lim) <= 1.0
    f = m0.reshape(-1)
    assert torch.equal(f[:255], _brd_mask(255, 1, p, 3).reshape(-1)), "the mask depends on the shape"


@pytest.mark.parametrize("N", H.COLSUM_NS)
@pytest.mark.parametrize("rows", H.COLSUM_ROWS)
def test_colsum_exact_on_integers_and_against_fp64(rows, N):
    g = H.gen(rows * 1000 + N)
    dy = H.draw(g, (rows, N), 8, 0.9)
    db0 = H.draw(g, (N,), 100, 1.0)
    H.need_exact(db0.abs() + dy.abs().sum(0), 1.0, "colsum")
    db = _g(N, db0.float())
    assert _lib().sm3_mlc_colsum(_P(_dev(dy.float())), _P(db), rows, N, None) == 0
    _done(db)
    H.same(db.t, db0 + dy.sum(0), "colsum on integers")
    dy, db0 = torch.randn(rows, N, generator=g), torch.randn(N, generator=g)
    db = _g(N, db0)
    assert _lib().sm3_mlc_colsum(_P(_dev(dy)), _P(db), rows, N, None) == 0
    _done(db)
    ref = db0.double() + dy.double().sum(0)
    lim = _sum_limit(db0.double().abs() + dy.double().abs().sum(0), rows + 1)
    assert H.record("colsum randn", float(((db.t.cpu().double() - ref).abs() / lim).max()), 1.0) <= 1.0


# ------------------------------------------------------------------------------------------------------------------------
# prototype heads
# ------------------------------------------------------------------------------------------------------------------------
def _heads_fwd(x, W, bias, tok, l2, lm):
    B, S, D = x.shape
    Tn = W.shape[0]
    out = _g(B * Tn)
    assert _lib().sm3_mlc_heads_fwd(_P(_dev(H.to_rows(x, lm))), _P(_dev(W)), _P(None if bias is None else _dev(bias)),
                                    _P(_dev(tok)), l2, _P(out), B, S, D, Tn, lm, None) == 0
    _done(out)
    return out.t.cpu().view(B, Tn)


W0, B0 = 2.0, -3.0   # dW / dbias start here: the kernels accumulate


def _heads_bwd(gl, x, W, bias, tok, l2, lm, det):
    from sm3hip import mlc
    B, S, D = x.shape
    Tn = W.shape[0]
    dx, dW = _g(B * S * D), _g(Tn * D, torch.full((Tn * D,), W0))
    db = None if bias is None else _g(Tn, torch.full((Tn,), B0))
    head = [_P(_dev(gl)), _P(_dev(H.to_rows(x, lm))), _P(_dev(W)), _P(_dev(tok)), l2, _P(dx), _P(dW), _P(db)]
    if det:
        work = torch.empty(mlc.heads_bwd_work(B, S, D, Tn, bias is not None), device=DEV)
        assert _lib().sm3_mlc_heads_bwd_det(*head, _P(work), B, S, D, Tn, lm, None) == 0
    else:
        assert _lib().sm3_mlc_heads_bwd(*head, B, S, D, Tn, lm, None) == 0
    _done(*([dx, dW] + ([] if db is None else [db])))
    return (H.from_rows(dx.t.cpu().view(B * S, D), B, S, lm), dW.t.cpu().view(Tn, D), None if db is None else db.t.cpu())


@pytest.mark.parametrize("lm", [0, 1])
@pytest.mark.parametrize("S,D,Tn,l2,hb", H.HEAD_CASES, ids=str)
def test_heads_forward_and_both_backward_forms_against_fp64(S, D, Tn, l2, hb, lm):
    x, W, bias, tok, gl = H.head_case(S, D, Tn, l2)
    bias = bias if hb else None
    r_out, r_dx, r_dW, r_db = H.head_apply(x, W, bias, tok, gl, l2, H.F64)
    lsc, wsc = H.head_out_scales(x, W, bias, tok, gl, l2)
    xsc, z = H.head_dx_scale(x, W, tok, gl, l2), H.head_zero_rows(x, l2)
    out = _heads_fwd(x, W, bias, tok, l2, lm)
    assert H.check_derived("head", None, "logits", out, r_out, lsc) <= 1.0
    if bool(z.any()):   # a zero row under l2: xn = 0, the logits of its prototypes are bias[t] exactly
        t0 = (tok.long() == S - 1)
        H.same(out[0, t0].to(DEV), bias[t0] if hb else torch.zeros(int(t0.sum())), "zero row: logits are the bias")
    forms = [_heads_bwd(gl, x, W, bias, tok, l2, lm, det) for det in (False, True)]
    for (dx, dW, db), form in zip(forms, ("atomic", "det")):
        assert H.check_derived("head", None, "dx", dx[~z], r_dx[~z], xsc[~z], tag=form) <= 1.0, form
        if bool(z.any()):
            assert H.check_derived("head", None, "dx0", dx[z], r_dx[z], xsc[z], tag=form) <= 1.0, form
        # W0 / B0 were added in fp32 and are subtracted here: they belong to the size of the sum
        assert H.check_derived("head", None, "dW", dW - W0, r_dW, wsc + W0, tag=form) <= 1.0, form
        if hb:
            assert H.check_derived("head", None, "dbias", db - B0, r_db, r_db.abs().max() + abs(B0), tag=form) <= 1.0, form
        if S >= 3:       # token 1 owns no prototype
            H.same(dx[:, 1].to(DEV), torch.zeros(x.shape[0], D), "dx of a token without prototypes")
    assert _bits(forms[0][0], forms[1][0]), "dx differs between the atomic and the fixed-order form"


@pytest.mark.parametrize("lm", [0, 1])
@pytest.mark.parametrize("S,D,Tn", [(3, 7, 31), (8, 33, 21), (1, 4096, 21), (8, 512, 33), (8, 31, 256)], ids=str)
def test_heads_backward_on_integers_is_exact(S, D, Tn, lm):
    g = H.gen(S * D + Tn)
    B = H.HEAD_B
    x, W, gl = H.draw(g, (B, S, D), 4, 0.9), H.draw(g, (Tn, D), 3, 0.9), H.draw(g, (B, Tn), 5, 0.9)
    tok = H.head_tokens(S, Tn)
    bias = H.draw(g, (Tn,), 7, 1.0)
    xt = x[:, tok.long()]
    H.need_exact(W0 + (gl.abs().unsqueeze(2) * xt.abs()).sum(0), 1.0, "dW")
    H.need_exact((xt.abs() * W.abs()).sum(2) + bias.abs(), 1.0, "logits")
    H.need_exact(gl.abs() @ W.abs(), 1.0, "dx")
    out = _heads_fwd(x.float(), W.float(), bias.float(), tok, 0, lm)
    H.same(out.to(DEV), (xt * W).sum(2) + bias, "logits on integers")
    for det in (False, True):
        dx, dW, db = _heads_bwd(gl.float(), x.float(), W.float(), bias.float(), tok, 0, lm, det)
        H.same(dW.to(DEV), W0 + torch.einsum("bt,btd->td", gl, xt), "dW on integers")
        H.same(db.to(DEV), B0 + gl.sum(0), "dbias on integers")
        want = torch.zeros(B, S, D, dtype=torch.float64).index_add_(1, tok.long(), gl.unsqueeze(2) * W)
        H.same(dx.to(DEV), want, "dx on integers")


# ------------------------------------------------------------------------------------------------------------------------
# refused arguments: SM3_EINVAL and not a byte written
# ------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_leave_every_output_untouched():
    lib = _lib()
    z = torch.zeros(8 * 9 * 3 * 72 + 4200 * 4, device=DEV)     # every input points here: large enough for each shape below
    zi = torch.zeros(512, dtype=torch.int32, device=DEV)
    o = [_g(8 * 9 * 3 * 72 + 4200 * 4) for _ in range(4)]
    I, O = _P(z), [_P(b) for b in o]
    N = _P(None)
    att_f = lambda B=2, S=8, D=64, nh=8, p=0.1, q=I, out=O[0]: lib.sm3_mlc_attention_fwd(q, out, B, S, D, nh, p, 1, 1, None)
    att_b = lambda B=2, S=8, D=64, nh=8, p=0.1, q=I, do=I, dq=O[0]: lib.sm3_mlc_attention_bwd(q, do, dq, B, S, D, nh, p, 1, 1, None)
    calls = []
    for f in (att_f, att_b):
        calls += [f(S=9), f(nh=9, D=72), f(D=66), f(p=1.0), f(p=-0.1), f(q=N), f(B=0), f(S=0)]
    calls += [att_f(out=N), att_b(do=N), att_b(dq=N)]
    ln_f = lambda a=I, b=I, g=I, be=I, p=0.1, out=O[0], st=O[1], rows=4, D=64: lib.sm3_mlc_add_ln_fwd(a, b, g, be, H.EPS, p, 1, out, st, rows, D, None)
    calls += [ln_f(D=4097), ln_f(p=1.0), ln_f(p=-0.1), ln_f(a=N), ln_f(b=N), ln_f(g=N), ln_f(be=N), ln_f(out=N), ln_f(st=N), ln_f(rows=0)]
    for det in (0, 1):
        def ln_b(do=I, a=I, b=I, st=I, g=I, p=0.1, da=O[0], db=O[1], dg=O[2], dbe=O[3], rows=4, D=64):
            if det:
                return lib.sm3_mlc_add_ln_bwd_det(do, a, b, st, g, p, 1, da, db, dg, dbe, None, rows, D, None)
            return lib.sm3_mlc_add_ln_bwd(do, a, b, st, g, p, 1, da, db, dg, dbe, rows, D, None)
        calls += [ln_b(D=4097), ln_b(p=1.0), ln_b(p=-0.1), ln_b(do=N), ln_b(a=N), ln_b(b=N), ln_b(st=N), ln_b(g=N), ln_b(da=N),
                  ln_b(db=N), ln_b(dg=N), ln_b(dbe=N), ln_b(rows=0)]
    brd = lambda y=I, b=I, p=0.1, h=O[0], hd=O[1], rows=4, n=7: lib.sm3_mlc_bias_relu_drop_fwd(y, b, p, 1, h, hd, rows, n, None)
    calls += [brd(p=1.0), brd(p=-0.1), brd(y=N), brd(b=N), brd(h=N), brd(hd=N), brd(rows=0), brd(n=0)]
    rdb = lambda d=I, h=I, p=0.1, dh=O[0], rows=4, n=7: lib.sm3_mlc_relu_drop_bwd(d, h, p, 1, dh, O[1], rows, n, None)
    calls += [rdb(p=1.0), rdb(p=-0.1), rdb(d=N), rdb(h=N), rdb(dh=N), rdb(rows=0)]
    calls += [lib.sm3_mlc_colsum(N, O[0], 4, 7, None), lib.sm3_mlc_colsum(I, N, 4, 7, None), lib.sm3_mlc_colsum(I, O[0], 0, 7, None),
              lib.sm3_mlc_colsum(I, O[0], 4, 0, None)]
    T = _P(zi)
    hf = lambda x=I, w=I, t=T, out=O[0], S=8: lib.sm3_mlc_heads_fwd(x, w, I, t, 1, out, 2, S, 16, 21, 1, None)
    calls += [hf(S=9), hf(x=N), hf(w=N), hf(t=N), hf(out=N)]
    for det in (0, 1):
        def hb(gl=I, x=I, w=I, t=T, dx=O[0], dw=O[1], S=8, Tn=21, work=I):
            if det:
                return lib.sm3_mlc_heads_bwd_det(gl, x, w, t, 1, dx, dw, O[2], work, 2, S, 16, Tn, 1, None)
            return lib.sm3_mlc_heads_bwd(gl, x, w, t, 1, dx, dw, O[2], 2, S, 16, Tn, 1, None)
        calls += [hb(Tn=257), hb(S=9), hb(gl=N), hb(x=N), hb(w=N), hb(t=N), hb(dx=N), hb(dw=N)]
        if det:
            calls += [hb(work=N)]
    torch.cuda.synchronize()
    assert all(rc == H.EINVAL for rc in calls), calls
    assert all(b.untouched() for b in o)
