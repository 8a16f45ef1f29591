"""GPU: the NT-Xent kernels (csrc/ntxent.hip) at their edges, against the fp64 oracle.

Inputs are clustered projections (tests/edge_inputs.py: positives at cosine ~ 1, same-cluster negatives at ~ 0.99,
optionally every row at its own scale from 1e-3 to 1e3) at temperatures down to 0.01, where the logits reach +-100 and
exp() overflows fp32 unless the maximum is subtracted; shapes from R = 2 (the only candidate is the positive) over
ragged anchor groups and candidate tiles to the row-per-workgroup fallback; dz in fp32, bf16 and f16.

Bounds (the fp32 tests' own, tests/test_kernels_gpu.py): loss within 2e-5 * max(1, |loss|); dz within
1e-4 * max|dz_ref| + 1e-7 per element, plus one rounding of a 16-bit output (|dz_ref| * 2^-8 bf16, 2^-10 f16).
tests/test_edge_refs_cpu.py shows the fp32 closed form inside half of both on the same inputs."""
import functools
import math

import numpy as np
import pytest
import torch

import edge_inputs as E

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16, torch.float16]
IDS = ["f32", "bf16", "f16"]
CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
DEV = "cuda:0"


def _ops():
    from sm3hip import ops
    return ops


@functools.lru_cache(maxsize=None)
def _case(R, D, kind, T, weight=1.0):
    """(z fp32, reference loss, reference gradient): computed once, shared by the tests, never written to."""
    if kind == "randn":
        z = torch.randn(R, D, generator=torch.Generator().manual_seed(R * 7 + D))
    else:
        z = E.clustered(R, D, seed=R * 1000 + D, row_scale=(kind == "scaled"))
    loss, grad = E.ntxent_ref(z, T, weight)
    return z, loss, grad


def _fused(z, T, weight, dt, scale=None, loss0=0.0, poison=False):
    ops = _ops()
    R, D = z.shape
    ws = torch.full((ops.ntxent_workspace_floats(R, D),), float("nan") if poison else 0.0, device=DEV)
    loss = torch.full((1,), loss0, device=DEV)
    dz = torch.full((R, D), float("nan"), dtype=dt, device=DEV)
    ops.ntxent_fused(CODE[dt], z.to(DEV), T, weight, ws, loss, dz,
                     dz_scale=None if scale is None else torch.tensor([scale], device=DEV))
    torch.cuda.synchronize()
    return float(loss), dz.cpu(), ws.cpu()


def _check(tag, got_loss, got_dz, ref_loss, ref_dz, dt, scale=1.0):
    rl = E.record(f"ntxent loss ({tag})", abs(got_loss - ref_loss), E.loss_limit(ref_loss))
    lim = E.dz_limit(ref_dz, dt)
    rd = E.worst_ratio(got_dz.double() / scale, ref_dz, lim)
    E.record(f"ntxent dz {IDS[DT.index(dt)]} ({tag})", rd, 1.0)
    assert rl <= 1.0 and rd <= 1.0, (tag, dt, got_loss, ref_loss, rl, rd)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("R,D", E.NTX_SHAPES, ids=str)
def test_fused_on_clustered_rows_at_low_temperature(R, D, dt):
    """sm3_ntxent_fused, tiled (D % 4 == 0, D <= 128) and row path, every output type, T in {0.5, 0.07, 0.01}."""
    path = "tiled" if D % 4 == 0 and D <= 128 else "row"
    for T in E.NTX_TEMPS:
        for kind in ("clustered", "scaled"):
            z, ref_loss, ref_dz = _case(R, D, kind, T, 0.5)
            loss, dz, _ = _fused(z, T, 0.5, dt)
            _check(f"{path}, {kind}", loss, dz, ref_loss, ref_dz, dt)
    z, ref_loss, ref_dz = _case(R, D, "randn", 0.07, 0.5)
    loss, dz, _ = _fused(z, 0.07, 0.5, dt)
    _check(f"{path}, randn", loss, dz, ref_loss, ref_dz, dt)


@pytest.mark.parametrize("R,D", [(6, 128), (66, 128), (514, 128), (10, 130)], ids=str)
def test_fused_f16_with_a_loss_scale(R, D):
    """f16 dz under dz_scale = 1024 (unscaled rows: a row at scale 1e-3 times 1024 would leave f16's range)."""
    for T in E.NTX_TEMPS:
        z, ref_loss, ref_dz = _case(R, D, "clustered", T, 0.5)
        assert float(ref_dz.abs().max()) * 1024 < 60000
        loss, dz, _ = _fused(z, T, 0.5, torch.float16, scale=1024.0)
        _check("f16, dz_scale 1024", loss, dz, ref_loss, ref_dz, torch.float16, scale=1024.0)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("D", [128, 36, 130], ids=str)
def test_two_rows_give_exactly_zero(D, dt):
    """R = 2: the only candidate of a row is its positive, so the loss term is 0.0 and every dz element +-0 -- exactly.  A NaN
    here is 0 * inf or exp(-inf) gone wrong (62 of the 64 tile candidates are padding)."""
    for T in E.NTX_TEMPS:
        for kind in ("clustered", "scaled"):
            z, ref_loss, ref_dz = _case(2, D, kind, T, 1.0)
            assert ref_loss == 0.0 and float(ref_dz.abs().max()) < 1e-9
            loss, dz, _ = _fused(z, T, 1.0, dt, loss0=0.375)
            assert loss == 0.375, (T, kind, loss)
            assert bool((dz.float() == 0).all()), (T, kind, dz)


@pytest.mark.parametrize("R,D", [(10, 36), (66, 128), (10, 130)], ids=str)
def test_zero_row_follows_normalize_clamp(R, D):
    """A zero row: zn = 0, inv_norm = 1e12 (F.normalize's clamp, which the oracle has too).  Its own gradient is 1e12 times
    d(loss)/d(zn); every other row keeps the usual bound at its own scale."""
    ops = _ops()
    z = E.clustered(R, D, seed=R + D).clone()
    k = R // 2 + 1
    z[k] = 0
    ref_loss, ref_dz = E.ntxent_ref(z, 0.07)
    loss, dz, ws = _fused(z, 0.07, 1.0, torch.float32)
    zn, inv = ws[:R * D].view(R, D), ws[R * D:R * D + R]
    assert bool((zn[k] == 0).all()) and float(inv[k]) == float(np.float32(1.0) / np.float32(1e-12))
    _check("zero row", loss, dz, ref_loss, ref_dz, torch.float32)
    others = [i for i in range(R) if i != k]
    assert bool(torch.isfinite(dz).all())
    r = E.worst_ratio(dz[others], ref_dz[others], E.dz_limit(ref_dz[others]))
    assert E.record("ntxent dz f32 (zero row, the other rows)", r, 1.0) <= 1.0


@pytest.mark.parametrize("R,D", [(10, 36), (66, 128), (10, 130)], ids=str)
def test_identical_rows_that_are_not_a_pair(R, D):
    """Rows 0 and 1 bit-identical (not each other's positive): a negative at cosine exactly 1."""
    z = E.clustered(R, D, seed=R + D + 1).clone()
    z[1] = z[0]
    for T in (0.07, 0.01):
        ref_loss, ref_dz = E.ntxent_ref(z, T)
        loss, dz, _ = _fused(z, T, 1.0, torch.float32)
        _check("identical rows", loss, dz, ref_loss, ref_dz, torch.float32)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("R,D", [(6, 128), (10, 36), (66, 128), (514, 128), (10, 130)], ids=str)
def test_poisoned_buffers_are_fully_overwritten(R, D, dt):
    """dz and the workspace start as NaN, the loss accumulator at c: afterwards every dz element is written (a ragged anchor
    group skips no row) and loss == c + term."""
    z, ref_loss, ref_dz = _case(R, D, "clustered", 0.07, 0.5)
    c = 0.75
    loss, dz, ws = _fused(z, 0.07, 0.5, dt, loss0=c, poison=True)
    assert not bool(torch.isnan(dz.float()).any())
    assert not bool(torch.isnan(ws[:R * D + 3 * R]).any())
    _check("poisoned", loss - c, dz, ref_loss, ref_dz, dt)


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_logits_backward_and_normalize_backward_in_every_type(dt):
    """sm3_ntxent_logits -> sm3_ce_label0 -> sm3_ntxent_logits_bwd<T>, and sm3_normalize_rows_bwd<T>, against fp64."""
    ops = _ops()
    from oracle import sm3_oracle as O
    R, D, T = 66, 128, 0.07
    z, ref_loss, ref_dz = _case(R, D, "clustered", T, 0.5)
    zd = z.to(DEV)
    zn, inv = torch.empty(R, D, device=DEV), torch.empty(R, device=DEV)
    logits = torch.full((R, R - 1), float("nan"), device=DEV)
    ops.ntxent_logits(zd, T, zn, inv, logits)
    loss, dlog = torch.zeros(1, device=DEV), torch.empty(R, R - 1, device=DEV)
    ops.ce_label0(logits, 0.5, loss, dlog)
    dz = torch.full((R, D), float("nan"), dtype=dt, device=DEV)
    ops.ntxent_logits_bwd(CODE[dt], dlog, zn, inv, T, dz)
    torch.cuda.synchronize()
    ref_logits, _ = O.ntxent_logits(z.double(), E.f32(T))
    r = E.record("ntxent logits", (logits.cpu().double() - ref_logits).abs().max(), 2e-5)
    assert r <= 1.0
    _check("logits + ce + logits_bwd", float(loss), dz.cpu(), ref_loss, ref_dz, dt)

    # normalize_rows_bwd: dz = inv_norm * (v - zn (zn . v)) with v = a + b
    g = torch.Generator().manual_seed(5)
    zs = E.clustered(R, D, seed=77, row_scale=True)
    a, b = torch.randn(R, D, generator=g), torch.randn(R, D, generator=g)
    z64 = zs.double().requires_grad_(True)
    zn64 = z64 / z64.norm(dim=1, keepdim=True).clamp_min(1e-12)
    (zn64 * (a.double() + b.double())).sum().backward()
    ops.normalize_rows(zs.to(DEV), zn, inv)
    for second in (b, None):
        if second is None:
            z64.grad = None
            zn64 = z64 / z64.norm(dim=1, keepdim=True).clamp_min(1e-12)
            (zn64 * a.double()).sum().backward()
        # per row: the rows of this input differ in scale by 1e6, and a row's error is relative to its own gradient
        out = torch.full((R, D), float("nan"), dtype=dt, device=DEV)
        ops.normalize_rows_bwd(CODE[dt], a.to(DEV), None if second is None else second.to(DEV), zn, inv, out)
        torch.cuda.synchronize()
        out = out.cpu()
        if dt == torch.float16:  # rows at scale 1e-3 have gradients of 1e3 * |v|: inside f16's range
            assert float(z64.grad.abs().max()) < 60000
        worst = max(E.worst_ratio(out[i], z64.grad[i], E.dz_limit(z64.grad[i], dt)) for i in range(R))
        assert E.record(f"normalize_rows_bwd {IDS[DT.index(dt)]}", worst, 1.0) <= 1.0


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_batched_terms_against_fp64_in_every_type(dt):
    """sm3_ntxent_fused_batch: four terms of one shape, different inputs and weights, each dz and the summed loss."""
    ops = _ops()
    R, D, T = 130, 128, 0.07
    weights = [1.0, 0.5, 0.25, 0.125]
    zs = [E.clustered(R, D, seed=500 + t, row_scale=(t == 1)) for t in range(4)]
    refs = [E.ntxent_ref(z, T, w) for z, w in zip(zs, weights)]
    ws = torch.full((ops.ntxent_batch_workspace_floats(4, R, D),), float("nan"), device=DEV)
    loss = torch.zeros(1, device=DEV)
    dzs = [torch.full((R, D), float("nan"), dtype=dt, device=DEV) for _ in range(4)]
    assert ops.ntxent_fused_batch(CODE[dt], [z.to(DEV) for z in zs], T, weights, ws, loss, dzs)
    torch.cuda.synchronize()
    total = sum(r[0] for r in refs)
    assert E.record("ntxent loss (batch of 4)", abs(float(loss) - total), E.loss_limit(total)) <= 1.0
    for t in range(4):
        r = E.worst_ratio(dzs[t].cpu(), refs[t][1], E.dz_limit(refs[t][1], dt))
        assert E.record(f"ntxent dz {IDS[DT.index(dt)]} (batch of 4)", r, 1.0) <= 1.0, t


@pytest.mark.parametrize("Rl,Rg", [(6, 18), (130, 390)], ids=str)
def test_rect_kernel_on_clustered_cosines(Rl, Rg):
    """sm3_ntxent_rect: local anchors against the gathered candidates, own block first, in the middle and last."""
    ops = _ops()
    D = 64
    blocks = [E.clustered(Rl, D, seed=900 + r).double() for r in range(Rg // Rl)]
    za = torch.cat(blocks)
    nrm = lambda t: t / t.norm(dim=1, keepdim=True)
    for blk in range(Rg // Rl):
        off = blk * Rl
        S = (nrm(blocks[blk]) @ nrm(za).t()).float()
        for T in (0.07, 0.01):
            S64 = S.double().requires_grad_(True)
            ref = E.rect_loss_from_s(S64, off, E.f32(T), 0.5)
            ref.backward()
            ref = float(ref.detach())
            Sd = S.to(DEV)
            loss = torch.full((1,), 0.25, device=DEV)
            ops.ntxent_rect(Sd, off, T, 0.5, loss)
            torch.cuda.synchronize()
            rl = E.record("ntxent_rect loss", abs(float(loss) - 0.25 - ref), E.loss_limit(ref))
            rd = E.record("ntxent_rect dS", E.worst_ratio(Sd.cpu(), S64.grad, E.dz_limit(S64.grad)), 1.0)
            assert rl <= 1.0 and rd <= 1.0, (off, T, rl, rd)
            assert bool((Sd.cpu()[torch.arange(Rl), off + torch.arange(Rl)] == 0).all())


def test_ce_label0_with_one_class_and_with_wide_logits():
    ops = _ops()
    logits = torch.tensor([[3.5], [-80.0]], device=DEV)
    loss, dlog = torch.full((1,), 0.5, device=DEV), torch.full((2, 1), float("nan"), device=DEV)
    ops.ce_label0(logits, 1.0, loss, dlog)
    torch.cuda.synchronize()
    assert float(loss) == 0.5 and bool((dlog == 0).all())
    g = torch.Generator().manual_seed(257)
    x = (torch.rand(6, 257, generator=g) * 200 - 100).float()
    x[1, 0], x[2, 0] = 100.0, -100.0
    x64 = x.double().requires_grad_(True)
    ref = 0.5 * (torch.logsumexp(x64, dim=1) - x64[:, 0]).mean()
    ref.backward()
    ref = float(ref.detach())
    loss, dlog = torch.zeros(1, device=DEV), torch.full((6, 257), float("nan"), device=DEV)
    ops.ce_label0(x.to(DEV), 0.5, loss, dlog)
    torch.cuda.synchronize()
    rl = E.record("ce_label0 loss", abs(float(loss) - ref), E.loss_limit(ref))
    rd = E.record("ce_label0 dlogits", E.worst_ratio(dlog.cpu(), x64.grad, E.dz_limit(x64.grad)), 1.0)
    assert rl <= 1.0 and rd <= 1.0, (rl, rd)
