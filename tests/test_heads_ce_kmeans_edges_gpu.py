"""GPU: the pseudo-label cross-entropy (sm3_mlc_ce) and the spherical k-means kernels (sm3_mlc_kmeans_assign, its fixed-order
form, sm3_mlc_kmeans_update) of csrc/heads_train.hip at their edges, called through the C ABI.

Cross-entropy: head widths with one-class heads, B * H on either side of the 256-thread stride, T down to 0.01, unit
and amplitude-10 logits, a dominant class (its softmax is 1 in fp32) and all-equal logits; loss and dlogits against fp64
(the project's figures at unit scale, 8 x the torch-fp32 restatement's error elsewhere: head_inputs.py), column sums,
run-to-run bits, exact zeros where the softmax is 1 by definition.  k-means: integer inputs, so every score and sum is
exact and the argmax (first maximum) is compared with fp64 with no case excluded."""
import ctypes as C

import pytest
import torch

import head_inputs as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
_KEEP = []


def _lib():
    from sm3hip import _lib as L
    return L.load()


def _P(t):
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p((t.t if isinstance(t, H.Guarded) else t).data_ptr())


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
# cross-entropy
# ------------------------------------------------------------------------------------------------------------------------
def _offsets(widths):
    off = [0]
    for n in widths:
        off.append(off[-1] + n)
    return torch.tensor(off, dtype=torch.int32)


def _ce(x, tg, widths, T, loss0=H.CE_LOSS0):
    """-> (loss as stored, fp32 tensor [1] on the CPU; dlogits [B, Tn] on the CPU)"""
    B, Tn = x.shape
    loss, dl = H.Guarded(1, F32, torch.tensor([loss0])), H.Guarded(B * Tn, F32)
    assert _lib().sm3_mlc_ce(_P(_dev(x)), _P(_dev(tg)), _P(_dev(_offsets(widths))), len(widths), B, Tn, T, _P(loss), _P(dl),
                             None) == 0
    _done(loss, dl)
    return loss.t.cpu(), dl.t.cpu().view(B, Tn)


@pytest.mark.parametrize("widths,B", H.CE_SHAPES, ids=str)
def test_ce_loss_and_dlogits_against_fp64(widths, B):
    Hn = len(widths)
    for T in H.CE_TS:
        for regime in H.CE_REGIMES:
            x, tg = H.ce_case(widths, B, regime, T)
            ref_loss, ref_d, _ = H.ce_apply(x, tg, widths, T, H.F64)
            loss, dl = _ce(x, tg, widths, T)
            loss2, dl2 = _ce(x, tg, widths, T)
            assert _bits(loss, loss2) and _bits(dl, dl2), "two runs differ"
            what, key, gs = (widths, B, T, regime), (regime, T), H.ce_grad_scale(B, Hn, T)
            got = torch.tensor([float(loss) - H.CE_LOSS0], dtype=H.F64)
            assert H.check_derived("ce", key, "loss", got, torch.tensor([ref_loss], dtype=H.F64)) <= 1.0, what
            assert H.check_derived("ce", key, "dlogits", dl, ref_d, gs) <= 1.0, what
            if regime in ("unit", "equal") and T >= 0.7:
                assert H.record("ce loss, existing figure", abs(float(got) - ref_loss), H.UNIT_LOSS) <= 1.0, what
                assert H.record("ce dlogits, existing figure", H.abs_err(dl, ref_d), H.ce_dlogits_unit(B, Hn, T)) <= 1.0, what
            # every head's columns sum to 0: within the element bound (at |ref| <= k / T) times the head width
            elem = H.derived("ce", key, "dlogits") * 2.0 * gs
            o = 0
            for n in widths:
                s = float(dl[:, o:o + n].double().sum(1).abs().max())
                assert H.record(f"ce dlogits head sum ({regime}, T {T})", s, elem * n) <= 1.0, (what, o)
                if n == 1:
                    H.same(dl[:, o].to(DEV), torch.zeros(B), "one-class head: dlogits")
                o += n


@pytest.mark.parametrize("T", H.CE_TS)
def test_ce_one_class_heads_contribute_exactly_nothing(T):
    for amp in (1.0, 30.0, 1000.0):
        x = amp * torch.randn(37, 3, generator=H.gen(int(amp)))
        tg = torch.zeros(3, 37, dtype=torch.int64)
        for loss0 in (0.0, H.CE_LOSS0):
            loss, dl = _ce(x, tg, (1, 1, 1), T, loss0)
            H.same(loss.to(DEV), torch.tensor([loss0]), "one-class heads: loss")
            H.same(dl.to(DEV), torch.zeros(37, 3), "one-class heads: dlogits")


@pytest.mark.parametrize("T", H.CE_TS)
def test_ce_term_of_a_dominant_target_is_not_negative(T):
    """One (b, h) pair per launch, loss starting at 0: the stored loss is that pair's term.  The target leads by 200 T at
    least, exp(-200) is 0 in fp32 and the softmax of the target is 1: the term is 0 or a positive round-off, never
    negative, and the target's gradient p - 1 is 0 or negative."""
    worst = 0.0
    for n in (2, 3, 5):
        for amp in (1.0, 30.0):
            g = H.gen(n * 100 + int(amp))
            for i in range(8):
                x = amp * torch.randn(1, n, generator=g)
                t = int(torch.randint(0, n, (1,), generator=g))
                x[0, t] = float(x.max()) + 200.0 * T + 1.0 + i
                loss, dl = _ce(x, torch.tensor([[t]]), (n,), T, 0.0)
                worst = min(worst, float(loss))
                assert float(loss) >= 0.0, (n, amp, i, float(loss))
                assert float(dl[0, t]) <= 0.0 and bool((dl[0] * (torch.arange(n) != t) >= 0).all()), (n, amp, i, dl)
    H.record(f"ce dominant-target term, most negative (T {T})", -worst, 0.0)


def test_ce_refuses_bad_arguments():
    lib = _lib()
    x, tg, off = torch.zeros(4, 9, device=DEV), torch.zeros(4, 4, dtype=torch.int64, device=DEV), _offsets((1, 5, 1, 2)).to(DEV)
    loss, dl = H.Guarded(1, F32), H.Guarded(36, F32)
    f = lambda x=x, tg=tg, off=off, Hn=4, B=4, Tn=9, T=0.7, loss=loss, dl=dl: lib.sm3_mlc_ce(_P(x), _P(tg), _P(off), Hn, B, Tn, T,
                                                                                                 _P(loss), _P(dl), None)
    calls = [f(x=None), f(tg=None), f(off=None), f(loss=None), f(dl=None), f(Hn=0), f(B=0), f(Tn=0), f(T=0.0), f(T=-1.0)]
    torch.cuda.synchronize()
    assert all(rc == H.EINVAL for rc in calls), calls
    assert loss.untouched() and dl.untouched()


# ------------------------------------------------------------------------------------------------------------------------
# k-means
# ------------------------------------------------------------------------------------------------------------------------
S0, C0 = 2.0, 5     # sums / counts start here: the kernels accumulate
SLAB = 256


def _assign(emb, cent, form):
    """form: 'atomic', 'det' or 'only' (sums and counts null) -> assign [N] int64, sums [K, D] or None, counts [K] or None (CPU)"""
    N, D = emb.shape
    K = cent.shape[0]
    a = H.Guarded(N, torch.int64)
    sums = None if form == "only" else H.Guarded(K * D, F32, torch.full((K * D,), S0))
    cnt = None if form == "only" else H.Guarded(K, torch.int32, torch.full((K,), C0, dtype=torch.int32))
    if form == "det":
        slabs = torch.empty(((N + SLAB - 1) // SLAB) * K * D, device=DEV)
        rc = _lib().sm3_mlc_kmeans_assign_det(_P(_dev(emb)), _P(_dev(cent)), _P(a), _P(sums), _P(cnt), _P(slabs), N, D, K, None)
    else:
        rc = _lib().sm3_mlc_kmeans_assign(_P(_dev(emb)), _P(_dev(cent)), _P(a), _P(sums), _P(cnt), N, D, K, None)
    assert rc == 0
    _done(*[b for b in (a, sums, cnt) if b is not None])
    return a.t.cpu(), None if sums is None else sums.t.cpu().view(K, D), None if cnt is None else cnt.t.cpu()


@pytest.mark.parametrize("K", H.KM_KS)
@pytest.mark.parametrize("D", H.KM_DS)
@pytest.mark.parametrize("N", H.KM_NS)
def test_kmeans_assign_is_the_first_maximum_and_sums_are_exact(N, D, K):
    emb, cent = H.km_case(N, D, K)
    H.km_exact(emb, cent)
    ref_a, ref_c, ref_s, _ = H.km_ref(emb, cent)
    for form in ("atomic", "det", "only"):
        a, sums, cnt = _assign(emb, cent, form)
        assert torch.equal(a, ref_a), (form, int((a != ref_a).sum()), "assignments differ from the first maximum in fp64")
        if form != "only":
            assert int((cnt - C0).sum()) == N and torch.equal((cnt - C0).long(), ref_c), form
            H.same(sums.to(DEV), S0 + ref_s, f"sums ({form})")


def _update(cent, sums, counts):
    K, D = cent.shape
    c = H.Guarded(K * D, F32, cent)
    assert _lib().sm3_mlc_kmeans_update(_P(c), _P(_dev(sums)), _P(_dev(counts.to(torch.int32))), K, D, None) == 0
    _done(c)
    return c.t.cpu().view(K, D)


@pytest.mark.parametrize("D", H.KM_DS)
def test_kmeans_update_ordinary_empty_and_zero_sum_clusters(D):
    g = H.gen(D)
    cent = torch.randn(4, D, generator=g)
    cent[1] = 3.0 * cent[1] / cent[1].norm()                 # the empty cluster's old centroid, not normalised
    sums = H.draw(g, (4, D), 9, 1.0).float()
    sums[2] = 0                                              # three members that cancel
    sums[0, 0] = 5.0                                         # never an all-zero ordinary cluster (D = 1)
    sums[3, 0] = -2.0
    counts = torch.tensor([7, 0, 3, 1])
    got = _update(cent, sums, counts)
    ref = H.km_update_ref(cent, sums, counts)
    assert bool(torch.isfinite(got).all())
    assert H.record("kmeans centroids", H.abs_err(got, ref), H.UNIT_CENT) <= 1.0
    H.same(got[2].to(DEV), torch.zeros(D), "a zero-sum cluster stays zero")
    assert abs(float(got[1].double().norm()) - 1.0) < H.UNIT_CENT and float((got[1] - cent[1] / 3.0).abs().max()) < H.UNIT_CENT


@pytest.mark.parametrize("N,D,K", [(413, 64, 8), (5, 65, 2), (413, 1, 2), (1, 512, 1)], ids=str)
def test_kmeans_e_then_m_step_against_fp64(N, D, K):
    emb, cent = H.km_case(N, D, K)
    _, sums, cnt = _assign(emb, cent, "det")
    got = _update(cent, sums - S0, cnt - C0)
    _, ref_c, ref_s, _ = H.km_ref(emb, cent)
    ref = H.km_update_ref(cent, ref_s, ref_c)
    assert bool(torch.isfinite(got).all())
    assert H.record("kmeans centroids", H.abs_err(got, ref), H.UNIT_CENT) <= 1.0


def test_kmeans_refuses_bad_arguments():
    lib = _lib()
    emb, cent = torch.zeros(8, 16, device=DEV), torch.zeros(2, 16, device=DEV)
    a, s, c = H.Guarded(8, torch.int64), H.Guarded(32, F32), H.Guarded(2, torch.int32)
    f = lambda e=emb, ce=cent, a=a, s=s, c=c, N=8, D=16, K=2: lib.sm3_mlc_kmeans_assign(_P(e), _P(ce), _P(a), _P(s), _P(c), N, D, K, None)
    d = lambda e=emb, ce=cent, a=a, s=s, c=c, N=8, D=16, K=2: lib.sm3_mlc_kmeans_assign_det(_P(e), _P(ce), _P(a), _P(s), _P(c), None,
                                                                                              N, D, K, None)
    u = lambda ce=s, s=emb, c=c, K=2, D=16: lib.sm3_mlc_kmeans_update(_P(ce), _P(s), _P(c), K, D, None)
    calls = [f(c=None), f(s=None), f(e=None), f(ce=None), f(a=None), f(N=0), f(D=0), f(K=0),
             d(c=None), d(s=None), d(e=None), d(ce=None), d(a=None), d(N=0), d(D=0), d(K=0), d(N=257),
             u(ce=None), u(s=None), u(c=None), u(K=0), u(D=0)]
    torch.cuda.synchronize()
    assert all(rc == H.EINVAL for rc in calls), calls
    assert a.untouched() and s.untouched() and c.untouched()
