"""GPU: the optimizer kernels (csrc/adamw.hip) at their edges.

* position independence, exact: K = 37 distinct (p, g, m, v) tuples tiled over n elements; the update is a pure
  per-element function, so element i of p, m and v must equal element i mod K of a reference launch bit for bit.  A
  skipped element, a second update at the float4 body / scalar tail / grid-sweep boundary or an overrun into the guard
  floats behind the buffer changes bits.  The same for sm3_ema_update.
* five unpadded steps against the fp64 oracle, p, m and v element-wise (bounds: tests/edge_inputs.py adamw_ratios;
  tests/test_edge_refs_cpu.py shows the formula in torch fp32 inside half of each).  The hyper-parameters cross the C
  ABI as fp32, so the oracle is handed those fp32 values.  v's relative bound 2^-19 has the floor FLT_MIN: for
  g = 1e-20 the term (1 - beta2) g^2 = 1e-43 is an fp32 subnormal, which has absolute precision only.
* the dynamic-loss-scale triple check_finite -> adamw_dynamic -> loss_scale_update through growth and backoff against
  a restatement of GradScaler.update, state compared exactly after every call.
* check_finite at the grid-sweep boundary, sticky flag; argument checks."""
import math

import numpy as np
import pytest
import torch

import edge_inputs as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENT = 123.25
SWEEP = 4096 * 256 * 4  # elements one grid sweep of the float4 body covers
HP = (E.ADAM["lr"], E.ADAM["beta1"], E.ADAM["beta2"], E.ADAM["eps"])


def _ops():
    from sm3hip import ops
    return ops


def _bits(t):
    return t.view(torch.int32)


def _tiled(src, n):
    """(whole buffer, its first n elements): src [K] tiled periodically, GUARD sentinel floats behind."""
    buf = torch.full((n + GUARD,), SENT, device=DEV)
    buf[:n] = src.to(DEV)[torch.arange(n, device=DEV) % src.numel()]
    return buf, buf[:n]


def _guards_ok(buf, n):
    return bool((buf[n:] == SENT).all())


_canon = {}


def _canonical(kind):
    """The K results from a launch of 4 K elements (float4 body only), checked against fp64 once."""
    if kind in _canon:
        return _canon[kind]
    ops = _ops()
    if kind == "adamw":
        p, g, m, v = (_tiled(t, 4 * 37)[1] for t in E.adamw_tuples())
        ops.adamw(p, g, m, v, *HP, 0.05, 3)
        torch.cuda.synchronize()
        out = tuple(t[:37].clone() for t in (p, m, v))
        p0, g0, m0, v0 = (t.double() for t in E.adamw_tuples())
        E.adamw_ref_step(p0, g0, m0, v0, 3, 0.05, 1.0)
        for got, want in zip(out, (p0, m0, v0)):
            assert torch.allclose(got.cpu().double(), want, rtol=1e-5, atol=1e-30), (got, want)
    else:
        t0, p0 = _ema_tuples()
        t, p = _tiled(t0, 4 * 37)[1], _tiled(p0, 4 * 37)[1]
        ops.ema_update(t, p, 0.99)
        torch.cuda.synchronize()
        out = (t[:37].clone(),)
        want = E.f32(0.99) * t0.double() + (1.0 - E.f32(0.99)) * p0.double()
        assert torch.allclose(out[0].cpu().double(), want, rtol=1e-5, atol=1e-30)
    _canon[kind] = out
    return out


def _ema_tuples():
    g = torch.Generator().manual_seed(38)
    t, p = torch.randn(37, generator=g), torch.randn(37, generator=g)
    t[:4] = torch.tensor([0.0, -0.0, 1e-30, 1e30])
    p[2:6] = torch.tensor([0.0, 1e30, -1e-30, 0.0])
    return t, p


N_POS = [1, 2, 3, 5, 1023, 1025, 100003, SWEEP + 7, 2 * SWEEP + 1027]


@pytest.mark.parametrize("n", N_POS)
def test_adamw_is_position_independent_bit_for_bit(n):
    ops = _ops()
    canon = _canonical("adamw")
    (bp, p), (bg, g), (bm, m), (bv, v) = (_tiled(t, n) for t in E.adamw_tuples())
    g0 = g.clone()
    ops.adamw(p, g, m, v, *HP, 0.05, 3)
    torch.cuda.synchronize()
    idx = torch.arange(n, device=DEV) % 37
    for name, got, want in zip("pmv", (p, m, v), canon):
        diff = _bits(got) != _bits(want)[idx]
        assert not bool(diff.any()), (name, n, diff.nonzero().flatten()[:8].tolist())
    assert torch.equal(_bits(g), _bits(g0))
    assert all(_guards_ok(b, n) for b in (bp, bg, bm, bv))


@pytest.mark.parametrize("n", N_POS)
def test_ema_update_is_position_independent_bit_for_bit(n):
    ops = _ops()
    (canon,) = _canonical("ema")
    t0, p0 = _ema_tuples()
    (bt, t), (bp, p) = _tiled(t0, n), _tiled(p0, n)
    pc = p.clone()
    ops.ema_update(t, p, 0.99)
    torch.cuda.synchronize()
    idx = torch.arange(n, device=DEV) % 37
    diff = _bits(t) != _bits(canon)[idx]
    assert not bool(diff.any()), (n, diff.nonzero().flatten()[:8].tolist())
    assert torch.equal(_bits(p), _bits(pc)) and _guards_ok(bt, n) and _guards_ok(bp, n)


@pytest.mark.parametrize("grad_scale,wd", [(1.0, 0.05), (0.125, 0.05), (1.0, 0.0), (0.125, 0.0)])
def test_adamw_five_unpadded_steps_against_fp64(grad_scale, wd):
    ops = _ops()
    n = 200003
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(1))
    grads = E.adamw_grads(n, 5, seed=2)
    pr, mr, vr = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    gsum = torch.zeros(n, dtype=torch.float64)
    for step, g in enumerate(grads, start=1):
        E.adamw_ref_step(pr, g.double(), mr, vr, step, wd, grad_scale)
        ops.adamw(p, g.to(DEV), m, v, *HP, wd, step, grad_scale)
        gsum += (g.double() * grad_scale).abs()
    torch.cuda.synchronize()
    rp, rm, rv = E.adamw_ratios(f"5 steps, grad_scale {grad_scale}, wd {wd}", p.cpu(), m.cpu(), v.cpu(), pr, mr, vr, gsum)
    assert rp <= 1.0 and rm <= 1.0 and rv <= 1.0, (rp, rm, rv)


def test_dynamic_loss_scale_sequence_with_growth_and_backoff():
    """clean, clean (scale grows), overflow (scale halves, tracker resets, no step counted, p / m / v untouched), ...
    The gradients handed in are the clean ones times the current scale, so the unscale is exercised."""
    ops = _ops()
    n, interval, wd = 1027, 2, 0.05
    script = "ccOcOOcccOcc"
    kinds = [float("inf"), float("-inf"), float("nan"), float("inf")]
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(3))
    clean = E.adamw_grads(n, len(script), seed=4)
    for g in clean:  # |g| * scale stays finite in fp32 and exact (powers of two)
        g.clamp_(-1e4, 1e4)
    scale = torch.tensor([1024.0], device=DEV)
    tracker, taken, found = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(3))
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pr, mr, vr = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    gsum = torch.zeros(n, dtype=torch.float64)
    r_scale, r_tracker, r_taken, n_over = 1024.0, 0, 0, 0
    seen_growth = seen_backoff = False
    for k, what in enumerate(script):
        g = clean[k] * r_scale
        assert bool(torch.isfinite(g).all())
        if what == "O":
            g[(k * 131) % n] = kinds[n_over % len(kinds)]
            n_over += 1
        before = [_bits(t).clone() for t in (p, m, v)]
        gd = g.to(DEV)
        ops.check_finite(gd, found)
        assert int(found) == (1 if what == "O" else 0)
        ops.adamw_dynamic(p, gd, m, v, *HP, wd, 1.0, scale, taken, found)
        ops.loss_scale_update(scale, found, tracker, taken, 2.0, 0.5, interval)
        torch.cuda.synchronize()
        if what == "O":  # GradScaler.update() after an overflow
            r_scale, r_tracker = r_scale * 0.5, 0
            seen_backoff = True
            assert all(torch.equal(b, _bits(t)) for b, t in zip(before, (p, m, v))), k
        else:
            E.adamw_ref_step(pr, clean[k].double(), mr, vr, r_taken + 1, wd, 1.0)
            gsum += clean[k].double().abs()
            r_taken += 1
            r_tracker += 1
            if r_tracker >= interval:
                r_scale, r_tracker = r_scale * 2.0, 0
                seen_growth = True
        got = (float(scale), int(tracker), int(taken), int(found))
        assert got == (r_scale, r_tracker, r_taken, 0), (k, what, got, (r_scale, r_tracker, r_taken, 0))
    assert seen_growth and seen_backoff and r_taken == script.count("c")
    rp, rm, rv = E.adamw_ratios("dynamic loss scale", p.cpu(), m.cpu(), v.cpu(), pr, mr, vr, gsum)
    assert rp <= 1.0 and rm <= 1.0 and rv <= 1.0, (rp, rm, rv)


@pytest.mark.parametrize("n", [1, 63, 65, 1048576, 1048577, 3000001])
def test_check_finite_finds_one_value_anywhere(n):
    ops = _ops()
    g = torch.randn(n, generator=torch.Generator().manual_seed(n))
    flt_max = float(np.finfo(np.float32).max)
    edge = torch.tensor([flt_max, -flt_max, 1e-45, -1e-40, -0.0, 0.0, 2.0 ** -126])
    g[:min(n, edge.numel())] = edge[:n]
    if n > 8:
        g[-3:] = torch.tensor([flt_max, 1e-45, -0.0])
    gd = g.to(DEV)
    found = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.check_finite(gd, found)
    assert int(found) == 0
    for pos in sorted({0, n - 1, 1048575, 1048576}):
        if pos >= n:
            continue
        for bad in (float("inf"), float("-inf"), float("nan")):
            keep = gd[pos].clone()
            gd[pos] = bad
            found.zero_()
            ops.check_finite(gd, found)
            assert int(found) == 1, (n, pos, bad)
            gd[pos] = keep
    # sticky: a raised flag survives a clean buffer (the trainer checks several buffers into one flag)
    found.fill_(1)
    ops.check_finite(gd, found)
    assert int(found) == 1
    found.zero_()
    ops.check_finite(gd, found)
    assert int(found) == 0


def test_argument_checks_refuse_without_touching_the_buffers():
    ops = _ops()
    from sm3hip._lib import SM3LibraryError
    n = 1024
    bufs = [torch.randn(n + 4, generator=torch.Generator().manual_seed(s)).to(DEV) for s in range(4)]
    bufs[3].abs_()
    keep = [_bits(b).clone() for b in bufs]
    same = lambda: all(torch.equal(k, _bits(b)) for k, b in zip(keep, bufs))
    for odd in range(4):  # each of p, g, m, v in turn starts one float off a 16-byte boundary
        args = [b[1:1 + n] if i == odd else b[:n] for i, b in enumerate(bufs)]
        with pytest.raises(SM3LibraryError, match="SM3_EALIGN"):
            ops.adamw(*args, *HP, 0.05, 1)
        found, sc, taken = (torch.zeros(1, dtype=torch.int32, device=DEV), torch.ones(1, device=DEV),
                            torch.zeros(1, dtype=torch.int32, device=DEV))
        with pytest.raises(SM3LibraryError, match="SM3_EALIGN"):
            ops.adamw_dynamic(*args, *HP, 0.05, 1.0, sc, taken, found)
        torch.cuda.synchronize()
        assert same()
    with pytest.raises(SM3LibraryError, match="SM3_EALIGN"):
        ops.ema_update(bufs[0][1:1 + n], bufs[1][:n], 0.99)
    args = [b[:n] for b in bufs]
    with pytest.raises(SM3LibraryError, match="SM3_EINVAL"):
        ops.adamw(*args, *HP, 0.05, 0)
    with pytest.raises(SM3LibraryError, match="SM3_EINVAL"):
        ops.adamw(*[b[:0] for b in bufs], *HP, 0.05, 1)
    found = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(SM3LibraryError, match="SM3_EINVAL"):
        ops.check_finite(bufs[0][:0], found)
    torch.cuda.synchronize()
    assert same() and int(found) == 0
