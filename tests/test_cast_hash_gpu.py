"""GPU: sm3_cast_to_f32, sm3_cast_from_f32 and sm3_weights_changed (tail of csrc/pool.hip), exactly.

The casts are the conversions every 16-bit epilogue uses; the bit-exact suites feed representable values, so rounding
is checked here: all 65 536 patterns upwards, and downwards every finite 16-bit value with the midpoint to its successor
(ties to even), the midpoint +- one fp32 ulp and the last fp32 below the successor, in both signs -- which includes f16's
overflow threshold 65 520, the ties into and inside its subnormals and bf16's overflow threshold -- plus fp32 subnormals,
infinities, zeros and NaNs.  The reference is the CPU's conversion; NaN compares as NaN.

The weight hash is sum_i (bits_i + 0x9E3779B97F4A7C15) (2 i + 1) mod 2^64, restated in numpy uint64; a missed change
would leave a frozen encoder on stale filter banks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CODE = {torch.bfloat16: 1, torch.float16: 2}
DT = [torch.bfloat16, torch.float16]
IDS = ["bf16", "f16"]
GUARD = 64


def _ops():
    from sm3hip import ops
    return ops


def _from_bits16(bits, dt):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint16).view(np.int16).copy()).view(dt)


def _from_bits32(bits):
    return torch.from_numpy(np.asarray(bits, dtype=np.uint32).view(np.int32).copy()).view(torch.float32)


def _same_or_both_nan(got, want):
    """Bit equality, NaN == NaN.  -> indices that differ"""
    nan = torch.isnan(want.float())
    ok = torch.where(nan, torch.isnan(got.float()), got.view(torch.int16 if got.element_size() == 2 else torch.int32) ==
                     want.view(torch.int16 if want.element_size() == 2 else torch.int32))
    return (~ok).nonzero().flatten()


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_cast_to_f32_on_every_bit_pattern(dt):
    ops = _ops()
    src = _from_bits16(np.arange(65536), dt)
    want = src.float()
    dst = torch.full((65536,), 7.0, device=DEV)
    ops.cast_to_f32(CODE[dt], src.to(DEV), dst)
    torch.cuda.synchronize()
    bad = _same_or_both_nan(dst.cpu(), want)
    assert bad.numel() == 0, [(hex(int(i)), float(dst[i]), float(want[i])) for i in bad[:8]]
    assert int(torch.isnan(want).sum()) in (254, 2046)  # the NaN patterns were among them


def _rounding_inputs(dt):
    """fp32 inputs around every finite non-negative value h of dt and its successor h+: h, the midpoint, the midpoint -+
    one fp32 ulp, h+ less one fp32 ulp; both signs.  The successor of the largest finite value counts as 2^emax+1, so its
    midpoint is the overflow threshold."""
    n_fin = 0x7F80 if dt == torch.bfloat16 else 0x7C00
    h = _from_bits16(np.arange(n_fin), dt).double()
    hp = torch.cat([h[1:], h[-1:] + (h[-1] - h[-2])])
    mid = ((h + hp) / 2).float()
    assert torch.equal(mid.double(), (h + hp) / 2)  # exact in fp32
    up, down = torch.full_like(mid, float("inf")), torch.zeros_like(mid)
    pos = torch.cat([h.float(), mid, torch.nextafter(mid, down), torch.nextafter(mid, up), torch.nextafter(hp.float(), down)])
    return torch.cat([pos, -pos])


def _special_inputs():
    bits = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000, 0x00008000, 0x00018000,
            0x00800000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF,
            0x7FFFFFFF, 0xFFFFFFFF, 0x7F80FFFF, 0x7FC10000]
    vals = torch.tensor([65504.0, 65519.996, 65520.0, 65520.004, 65536.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23),
                         2.0 ** -26, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 3.3895314e38, 3.3961775e38, 3.4e38])
    rnd = torch.randint(-2 ** 31, 2 ** 31 - 1, (100000,), generator=torch.Generator().manual_seed(16), dtype=torch.int64)
    return torch.cat([_from_bits32(bits), vals, -vals, rnd.to(torch.int32).view(torch.float32)])


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_cast_from_f32_rounds_to_nearest_even_everywhere(dt):
    ops = _ops()
    src = torch.cat([_rounding_inputs(dt), _special_inputs()])
    want = src.to(dt)
    if dt == torch.float16:  # the reference itself, at the points the description names
        at = lambda x: int(torch.tensor([x], dtype=torch.float32).to(dt).view(torch.int16))
        assert at(65504.0) == 0x7BFF and at(65519.996) == 0x7BFF and at(65520.0) == 0x7C00
        assert at(2.0 ** -25) == 0 and at(2.0 ** -25 * (1 + 2.0 ** -23)) == 1 and at(-0.0) == -0x8000
    else:
        at = lambda b: int(_from_bits32([b]).to(dt).view(torch.int16))
        assert at(0x7F7F7FFF) == 0x7F7F and at(0x7F7F8000) == 0x7F80 and at(0x3F808000) == 0x3F80 and at(0x3F818000) == 0x3F82
    dst = torch.zeros(src.numel(), dtype=dt, device=DEV)
    ops.cast_from_f32(CODE[dt], src.to(DEV), dst)
    torch.cuda.synchronize()
    bad = _same_or_both_nan(dst.cpu(), want)
    assert bad.numel() == 0, (bad.numel(), [(float(src[i]), hex(int(src[i].view(torch.int32)) & 0xFFFFFFFF),
                                             hex(int(dst[i].cpu().view(torch.int16)) & 0xFFFF),
                                             hex(int(want[i].view(torch.int16)) & 0xFFFF)) for i in bad[:8]])


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("n", [1, 255, 257, 2097152 + 3])
def test_casts_write_n_elements_and_nothing_behind(n, dt):
    ops = _ops()
    src = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 100
    half = torch.full((n + GUARD,), 3.0, dtype=dt, device=DEV)
    ops.cast_from_f32(CODE[dt], src.to(DEV), half[:n])
    back = torch.full((n + GUARD,), 5.0, device=DEV)
    ops.cast_to_f32(CODE[dt], half[:n], back[:n])
    torch.cuda.synchronize()
    want = src.to(dt)
    assert torch.equal(half[:n].cpu().view(torch.int16), want.view(torch.int16)) and bool((half[n:] == 3.0).all())
    assert torch.equal(back[:n].cpu(), want.float()) and bool((back[n:] == 5.0).all())


def _hash(flat):
    bits = flat.cpu().numpy().view(np.uint32).astype(np.uint64)
    i = np.arange(bits.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(((bits + np.uint64(0x9E3779B97F4A7C15)) * (np.uint64(2) * i + np.uint64(1))).sum(dtype=np.uint64))


def test_hash_restatement_wraps_like_uint64():
    """CPU-side sanity of the reference (runs with the GPU tests: it needs nothing from the library)."""
    flat = torch.tensor([0.0, 1.0, -1.0])
    c = 0x9E3779B97F4A7C15
    want = (c * 1 + (0x3F800000 + c) * 3 + (0xBF800000 + c) * 5) % 2 ** 64
    assert _hash(flat) == want


@pytest.mark.parametrize("n", [1, 63, 64, 257, 262144, 262145, 3 * 262144 + 77])
def test_weights_changed_sees_every_single_change(n):
    ops = _ops()
    flat = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(DEV)
    bits = flat.view(torch.int32)
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    changed = torch.full((1,), -1, dtype=torch.int32, device=DEV)

    def call():
        ops.weights_changed(flat, state, changed)
        torch.cuda.synchronize()
        st = state.cpu().numpy().view(np.uint64)
        assert int(st[0]) == 0 and int(st[1]) == _hash(flat), (n, st)
        return int(changed)

    assert call() == 1  # against the all-zero state of a first call
    assert call() == 0

    def expect_seen(what):
        assert call() == 1, (n, what)
        assert call() == 0, (n, what)

    for i in sorted(i for i in {0, n - 1, 262144} if i < n):
        bits[i] ^= 1  # the lowest mantissa bit
        expect_seen(("bit flip", i))
    if n > 1:
        i, j = 0, n - 1
        assert int(bits[i]) != int(bits[j])
        flat[[i, j]] = flat[[j, i]]
        expect_seen("swap of the first and last element")
    if n > 262144 + 5:
        i, j = 5, 262144 + 5  # one grid stride apart: the same thread reads both
        flat[[i, j]] = flat[[j, i]]
        expect_seen("swap one grid stride apart")
    k = n // 2
    bits[k] = 0
    call()
    bits[k] = -2 ** 31  # +0.0 -> -0.0
    expect_seen("sign of zero")
    bits[k] = 0x7FC00000
    call()
    bits[k] = 0x7FC00001
    expect_seen("NaN payload")
