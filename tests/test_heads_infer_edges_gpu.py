"""GPU: the three inference kernels of the multi-label heads (csrc/heads.hip: sm3_token_attention, sm3_add_layernorm,
sm3_token_heads) in f32, bf16 and f16 at the edge shapes of the training suite, through sm3hip.ops.

The reference is fp64 on the 16-bit values of the inputs; a 16-bit output adds one rounding of its store to the bound
(|ref| * 2^-8 bf16, 2^-10 f16, as edge_inputs.HALF_ULP).  Bounds: head_inputs.py."""
import ctypes as C

import pytest
import torch

import head_inputs as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _ops():
    from sm3hip import ops
    return ops


def _ratio(got, ref, limit):
    return H.worst_ratio(got, ref.double(), limit)


def _derived_limit(family, regime, quantity, ref, dt, scale=None):
    """Element-wise: the derived bound in rel_err()'s measure, plus one rounding of a 16-bit store."""
    ref = ref.double()
    s = ref.abs().max() if scale is None else scale
    return H.derived(family, regime, quantity) * (s + ref.abs()) + ref.abs() * H.HALF_ULP[dt] + 1e-300


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("B", H.ATT_BS)
@pytest.mark.parametrize("S,D,nhead", H.ATT_CASES, ids=str)
def test_token_attention_against_fp64(S, D, nhead, B, dt):
    for regime in H.ATT_REGIMES:
        qkv = H.att_case(S, D, nhead, B, regime)[0].to(dt)
        ref, _ = H.att_apply(qkv, None, nhead, None, 0.0, H.F64)
        out = H.Guarded(B * S * D, dt)
        _ops().token_attention(CODE[dt], qkv.reshape(B * S, 3 * D).to(DEV), out.t, B, S, D, nhead)
        torch.cuda.synchronize()
        assert out.guards()
        got = out.t.cpu().view(B, S, D)
        what = (S, D, nhead, B, regime)
        r = _ratio(got, ref, _derived_limit("att", regime, "out", ref, dt))
        assert H.record(f"token_attention {IDS[DT.index(dt)]} ({regime})", r, 1.0) <= 1.0, what
        if regime != "peaked":
            r = _ratio(got, ref, H.half_limit(ref, H.UNIT_OUT, dt))
            assert H.record(f"token_attention {IDS[DT.index(dt)]}, existing figure ({regime})", r, 1.0) <= 1.0, what
        if S == 1:   # one candidate: out is V, whatever the type
            H.same(out.t, qkv[..., 2 * D:], "S = 1: out is V")


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("rows", H.LN_ROWS)
@pytest.mark.parametrize("D", H.LN_INFER_DS)
def test_add_layernorm_against_fp64(D, rows, dt):
    for regime in H.LN_REGIMES:
        a, b, gamma, beta, _ = H.ln_case(rows, D, regime)
        a, b = a.to(dt), b.to(dt)
        for bb in (b, None):
            ref = H.ln_apply(a, bb, gamma, beta, None, None, 0.0, H.F64)["out"]
            out = H.Guarded(rows * D, dt)
            _ops().add_layernorm(CODE[dt], a.to(DEV), None if bb is None else bb.to(DEV), gamma.to(DEV), beta.to(DEV), H.EPS, out.t,
                                 rows, D)
            torch.cuda.synchronize()
            assert out.guards()
            got = out.t.cpu().view(rows, D)
            what = (D, rows, regime, bb is None)
            r = _ratio(got, ref, _derived_limit("ln", (regime, D), "out", ref, dt))
            assert H.record(f"add_layernorm {IDS[DT.index(dt)]} ({regime})", r, 1.0) <= 1.0, what
            if regime == "unit":
                r = _ratio(got, ref, H.half_limit(ref, H.UNIT_OUT, dt))
                assert H.record(f"add_layernorm {IDS[DT.index(dt)]}, existing figure", r, 1.0) <= 1.0, what
            if regime == "const" and (D & (D - 1)) == 0:
                H.same(out.t, beta.to(dt).expand(rows, D), "constant row: out is beta, rounded to the output type")


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("S,D,Tn,l2", sorted({c[:4] for c in H.HEAD_CASES}), ids=str)   # the bias is not optional here
def test_token_heads_against_fp64(S, D, Tn, l2, dt):
    x, W, bias, tok, _ = H.head_case(S, D, Tn, l2)
    x = x.to(dt)
    B = x.shape[0]
    ref = H.head_apply(x, W, bias, tok, None, l2, H.F64)[0]
    lsc, _ = H.head_out_scales(x, W, bias, tok, torch.zeros(B, Tn), l2)
    out = H.Guarded(B * Tn, torch.float32)
    _ops().token_heads(CODE[dt], x.reshape(B * S, D).to(DEV), W.to(DEV), bias.to(DEV), tok.to(DEV), l2, out.t, B, S, D, Tn)
    torch.cuda.synchronize()
    assert out.guards()
    got = out.t.cpu().view(B, Tn)
    r = _ratio(got, ref, H.derived("head", None, "logits") * (lsc + ref.abs()) + 1e-300)
    assert H.record(f"token_heads {IDS[DT.index(dt)]}", r, 1.0) <= 1.0
    if l2 and S >= 3:    # x[0, S - 1] is all zero: xn = 0 and the logits of its prototypes are bias[t] exactly
        t0 = tok.long() == S - 1
        H.same(got[0, t0].to(DEV), bias[t0], "zero row: logits are the bias")


def test_refused_arguments_leave_every_output_untouched():
    from sm3hip import _lib as L
    lib, ops = L.load(), _ops()
    P = lambda t: C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())
    z = torch.zeros(9 * 3 * 1032, device=DEV)
    zi = torch.zeros(64, dtype=torch.int32, device=DEV)
    o = H.Guarded(9 * 1032, torch.float32)
    I, O, N = P(z), P(o.t), None
    ta = lambda q=I, out=O, B=1, S=8, D=64, nh=8: lib.sm3_token_attention(0, q, out, B, S, D, nh, None)
    ln = lambda a=I, g=I, be=I, out=O, rows=4, D=64: lib.sm3_add_layernorm(0, a, I, g, be, H.EPS, out, rows, D, None)
    th = lambda x=I, w=I, b=I, t=P(zi), out=O, S=8: lib.sm3_token_heads(0, x, w, b, t, 1, out, 1, S, 16, 21, None)
    calls = [ta(S=9), ta(nh=9, D=72), ta(D=66), ta(q=P(N)), ta(out=P(N)), ta(B=0),
             ln(D=1025), ln(a=P(N)), ln(g=P(N)), ln(be=P(N)), ln(out=P(N)), ln(rows=0),
             th(S=9), th(x=P(N)), th(w=P(N)), th(b=P(N)), th(t=P(N)), th(out=P(N))]
    torch.cuda.synchronize()
    assert all(rc == H.EINVAL for rc in calls), calls
    with pytest.raises(ValueError):
        ops.add_layernorm(0, z[:1025], None, z[:1025], z[:1025], H.EPS, o.t[:1025], 1, 1025)
    with pytest.raises(ValueError):
        ops.token_attention(0, z[:9 * 3 * 64], o.t[:9 * 64], 1, 9, 64, 8)
    torch.cuda.synchronize()
    assert o.untouched()
