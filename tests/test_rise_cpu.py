"""CPU: RISE saliency maps (sm3hip/rise.py, csrc/rise.hip) -- the numpy restatement of the three kernels (mask table, masked
inputs, weighted accumulation) that tests/test_rise_gpu.py compares the device against bit for bit, pinned here to the
definition by fixed vectors, range checks and hand-made tables; the definition as an estimator (mean mask, a planted block);
the entry points in the header, the binding and the library and their host-side refusals; the driver's and the four tools'
refusals (each before anything touches the GPU)."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]
ENTRY_POINTS = ("sm3_rise_table", "sm3_rise_compose", "sm3_rise_accumulate")
ROW = 36  # words of a table row: 32 of grid bits, oy, ox, two of padding


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- numpy restatements of the kernels (used by tests/test_rise_gpu.py) -------------------------------------------------
def philox4x32_10(ctr, key):
    """ctr: 4 uint32 arrays (broadcastable), key: (k0, k1) -> 4 uint32 arrays.  As csrc/attr.hip."""
    c = [np.asarray(v, np.uint64) & np.uint64(0xFFFFFFFF) for v in np.broadcast_arrays(*ctr)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        n0, n2 = (p1 >> np.uint64(32)) ^ c[1] ^ k0, (p0 >> np.uint64(32)) ^ c[3] ^ k1
        c = [n0, p1 & m32, n2, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return [v.astype(np.uint32) for v in c]


def cell_size(H, W, s):
    return -(-H // s), -(-W // s)


def threshold(p):
    return int(float(p) * 4294967296.0)


def table(seed, m, i0, c, H, W, s, p):
    """sm3_rise_table: [c, 36] uint32 rows of masks i0 .. i0 + c - 1 of modality m."""
    G, (ch, cw), thr = s + 2, cell_size(H, W, s), threshold(p)
    assert thr > 0
    key = (seed & 0xFFFFFFFF, seed >> 32)
    ncall = -(-G * G // 4)
    i = np.arange(i0, i0 + c, dtype=np.uint64)[:, None]
    w = philox4x32_10((np.arange(ncall + 1, dtype=np.uint64)[None, :], i, np.uint64(m), np.uint64(1)), key)  # 4 x [c, ncall + 1]
    words = np.stack(w, axis=2)                                                                              # [c, ncall + 1, 4]
    bits = words[:, :ncall].reshape(c, -1)[:, :G * G] < np.uint32(thr)
    out = np.zeros((c, ROW), np.uint32)
    for j in range(G * G):
        out[:, j >> 5] |= bits[:, j].astype(np.uint32) << np.uint32(j & 31)
    out[:, 32] = (words[:, ncall, 0].astype(np.uint64) * np.uint64(ch)) >> np.uint64(32)
    out[:, 33] = (words[:, ncall, 1].astype(np.uint64) * np.uint64(cw)) >> np.uint64(32)
    return out


def grid_bits(row, s):
    """[G, G] 0 / 1 of a table row."""
    G = s + 2
    j = np.arange(G * G)
    return ((row[j >> 5] >> (j & 31).astype(np.uint32)) & 1).astype(np.int64).reshape(G, G)


def mask_A(row, H, W, s, check=False):
    """The integer A [H, W] of a table row."""
    (ch, cw), g = cell_size(H, W, s), grid_bits(row, s)
    oy, ox = int(row[32]), int(row[33])
    Y, X = np.arange(H)[:, None] + oy, np.arange(W)[None, :] + ox
    gy, ry, gx, rx = Y // ch, Y % ch, X // cw, X % cw
    if check:
        assert 0 <= oy < ch and 0 <= ox < cw and gy.max() + 1 <= s + 1 and gx.max() + 1 <= s + 1
    return ((ch - ry) * (cw - rx) * g[gy, gx] + (ch - ry) * rx * g[gy, gx + 1] + ry * (cw - rx) * g[gy + 1, gx] +
            ry * rx * g[gy + 1, gx + 1])


def mask_of(row, H, W, s):
    """[H, W] f32: (float)A / (float)(ch * cw), one correctly rounded division."""
    ch, cw = cell_size(H, W, s)
    return mask_A(row, H, W, s).astype(np.float32) / np.float32(ch * cw)


def masks_of(tab, H, W, s):
    return np.stack([mask_of(row, H, W, s) for row in tab])


def blend(x, b, a):
    """fadd(b, fmul(a, fsub(x, b))): three separately rounded f32 operations."""
    x, b, a = np.float32(x), np.float32(b), np.float32(a)
    with np.errstate(all="ignore"):
        return (b + (a * (x - b)).astype(np.float32)).astype(np.float32)


def compose(x, base, tab, H, W, s):
    """sm3_rise_compose: x [N, 3, H, W], base [1 | N, 3, H, W], tab [c, 36] -> [c, N, 3, H, W]."""
    mk = masks_of(tab, H, W, s)
    return blend(x[None], np.broadcast_to(base, x.shape)[None], mk[:, None, None])


def accumulate(tab, weights, H, W, s, p):
    """sm3_rise_accumulate: weights [M, R] f32 -> [R, H, W] f32, ascending i, product and sum rounded on their own, / d."""
    M, R = weights.shape
    acc = np.zeros((R, H, W), np.float32)
    with np.errstate(all="ignore"):
        for i in range(M):
            acc = (acc + (np.float32(weights[i])[:, None, None] * mask_of(tab[i], H, W, s)[None]).astype(np.float32)).astype(
                np.float32)
        return (acc / np.float32(float(M) * float(p))).astype(np.float32)


# ---- the restatement against the definition's fixed vectors -----------------------------------------------------------------
def test_philox_known_answer():
    w = philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(v) for v in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_fixed_vectors_of_the_definition():
    t = table(12345, 0, 0, 4, 224, 224, 7, 0.5)
    assert cell_size(224, 224, 7) == (32, 32)
    assert t[:, 32].tolist() == [0, 4, 5, 27] and t[:, 33].tolist() == [12, 17, 15, 8]
    assert "".join(map(str, grid_bits(t[0], 7).reshape(-1))) == \
        "110010011110100111010110110011010111110101010111001001000111001000111000101101111"
    assert [int(mask_A(r, 224, 224, 7).sum()) for r in t] == [28028928, 24797600, 22682800, 25343536]
    m0 = mask_of(t[0], 224, 224, 7)
    assert m0.dtype == np.float32 and (float(m0[0, 0]), float(m0[223, 223]), float(m0[112, 74])) == (1.0, 0.0107421875, 0.5)
    assert not t[:, 34:].any()

    t = table(2 ** 40 + 3, 1, 0, 4, 30, 34, 4, 0.25)
    assert cell_size(30, 34, 4) == (8, 9)
    assert t[:, 32].tolist() == [2, 0, 7, 3] and t[:, 33].tolist() == [4, 2, 1, 1]
    assert "".join(map(str, grid_bits(t[0], 4).reshape(-1))) == "100000100001100000011000001000000000"
    assert [int(mask_A(r, 30, 34, 4).sum()) for r in t] == [14535, 17260, 7974, 28395]
    m0 = mask_of(t[0], 30, 34, 4)
    assert (float(m0[0, 0]), float(m0[29, 33]), float(m0[15, 11])) == (0.5555555820465088, 0.0, 0.125)
    # a row is a function of the mask index alone, not of the call's i0 and c
    assert np.array_equal(table(2 ** 40 + 3, 1, 2, 2, 30, 34, 4, 0.25), t[2:])
    assert not np.array_equal(table(2 ** 40 + 3, 0, 0, 4, 30, 34, 4, 0.25), t)


@pytest.mark.parametrize("H,W,s", [(224, 224, 7), (64, 64, 7), (32, 32, 4), (64, 96, 5), (30, 34, 7), (448, 448, 14), (8, 8, 8),
                                   (4, 4, 1)])
def test_every_index_and_value_is_in_range(H, W, s):
    ch, cw = cell_size(H, W, s)
    tab = table(99, 1, 0, 64, H, W, s, 0.5)
    for row in tab:
        A = mask_A(row, H, W, s, check=True)                                      # grid indices and shifts
        assert A.min() >= 0 and A.max() <= ch * cw
        m = mask_of(row, H, W, s)
        assert m.min() >= 0.0 and m.max() <= 1.0
    G = s + 2
    used = np.zeros(32, np.uint32)
    for j in range(G * G):
        used[j >> 5] |= np.uint32(1) << np.uint32(j & 31)
    assert not (tab[:, :32] & ~used).any()                                        # no bit beyond G * G


def _hand_row(s, bits, oy=0, ox=0):
    row = np.zeros(ROW, np.uint32)
    for j in bits:
        row[j >> 5] |= np.uint32(1) << np.uint32(j & 31)
    row[32], row[33] = oy, ox
    return row


def test_mask_function_on_hand_made_tables():
    H, W, s = 12, 20, 4
    ch, cw, G = 3, 5, 6
    full = _hand_row(s, range(G * G), 2, 3)
    assert np.array_equal(mask_of(full, H, W, s), np.ones((H, W), np.float32))
    assert np.array_equal(mask_of(_hand_row(s, [], 1, 4), H, W, s), np.zeros((H, W), np.float32))
    ramp = mask_of(_hand_row(s, [0]), H, W, s)
    want = np.zeros((H, W), np.float32)
    for y in range(ch):
        for x in range(cw):
            want[y, x] = np.float32((ch - y) * (cw - x)) / np.float32(ch * cw)
    assert np.array_equal(ramp, want) and ramp[0, 0] == 1.0 and ramp[ch - 1, cw - 1] == np.float32(1) / np.float32(15)
    # the shift moves the ramp: with oy = 1, ox = 2 pixel (0, 0) sits at (1, 2) of the first cell
    moved = mask_of(_hand_row(s, [0], 1, 2), H, W, s)
    assert moved[0, 0] == np.float32((ch - 1) * (cw - 2)) / np.float32(15) and np.array_equal(moved[:2, :3], want[1:3, 2:5])


def test_compose_and_accumulate_by_hand():
    H, W, s = 2, 2, 1                                                             # one cell of 2 x 2, G = 3
    x = np.float32([[[[1, 2], [3, 4]], [[5, 6], [7, 8]], [[-1, -2], [-3, -4]]]])  # [1, 3, 2, 2]
    b = np.float32(0.5) * np.ones((1, 3, 2, 2), np.float32)
    tab = np.stack([_hand_row(s, [0]), _hand_row(s, [0, 3], 1, 0)])
    m0, m1 = mask_of(tab[0], H, W, s), mask_of(tab[1], H, W, s)
    assert np.array_equal(m0, np.float32([[1, 0.5], [0.5, 0.25]])) and np.array_equal(m1, np.float32([[1, 0.5], [1, 0.5]]))
    out = compose(x, b, tab, H, W, s)
    assert out.shape == (2, 1, 3, 2, 2) and out.dtype == np.float32
    assert np.array_equal(out[0, 0, 0], np.float32([[1, 1.25], [1.75, 1.375]]))   # 0.5 + m (x - 0.5)
    assert np.array_equal(out[1, 0, 2], np.float32([[-1, -0.75], [-3, -1.75]]))
    w = np.float32([[0.5, 1.0], [0.25, 0.0]])                                     # [M = 2, R = 2]
    got = accumulate(tab, w, H, W, s, 0.5)                                        # d = 1
    assert np.array_equal(got[0], np.float32(0.5) * m0 + np.float32(0.25) * m1) and np.array_equal(got[1], m0)
    assert np.array_equal(accumulate(tab, w, H, W, s, 0.25)[1], m0 / np.float32(0.5))
    # -0, NaN and inf go through the three operations, not a shortcut: mask 1 keeps x, mask 0 gives b + 0 * (x - b)
    odd = np.float32([[[[-0.0, np.inf], [np.nan, 1.0]]] * 3])
    ones, zeros = _hand_row(s, range(9)), _hand_row(s, [])
    got = compose(odd, np.zeros((1, 3, 2, 2), np.float32), np.stack([ones, zeros]), H, W, s)
    assert np.signbit(got[0, 0, 0, 0, 0]) == False and got[0, 0, 0, 0, 1] == np.inf  # noqa: E712  (0 + 1 * (-0 - 0) = +0)
    assert np.isnan(got[1, 0, 0, 0, 1]) and np.isnan(got[1, 0, 0, 1, 0]) and got[1, 0, 0, 1, 1] == 0.0


# ---- the definition is a sensible estimator -----------------------------------------------------------------------------
def test_the_mean_mask_is_the_keep_probability():
    """Seed 7, m 1, 224^2, s 7, p 0.5, M 4000: the per-pixel mean of the masks; measured [0.4884, 0.5159]."""
    H = W = 224
    tab = table(7, 1, 0, 4000, H, W, 7, 0.5)
    total = np.zeros((H, W), np.int64)
    for row in tab:
        total += mask_A(row, H, W, 7)
    mean = total / (4000.0 * 32 * 32)
    print(f"mean mask in [{mean.min():.4f}, {mean.max():.4f}]")
    assert 0.47 <= mean.min() and mean.max() <= 0.53


def _faith_ranks(m):
    order = np.argsort(-m.reshape(-1), kind="stable")                             # descending, ties by ascending index
    return order


def test_a_planted_block_is_found():
    """32 x 32, s 4, M 2000, p 0.5; a linear score with weight 1.0 on a random 8 x 8 block and 0.02 U[0, 1) elsewhere, squashed by
    a logistic of its z-value over the M scores; 20 trials."""
    H = W = 32
    g = np.random.default_rng(5)
    shares = []
    for trial in range(20):
        by, bx = int(g.integers(0, H - 8 + 1)), int(g.integers(0, W - 8 + 1))
        w = 0.02 * g.random((H, W))
        w[by:by + 8, bx:bx + 8] += 1.0
        x = 0.5 + g.random((H, W))
        tab = table(1000 + trial, 0, 0, 2000, H, W, 4, 0.5)
        mk = masks_of(tab, H, W, 4)
        score = (mk.astype(np.float64) * (w * x)[None]).sum(axis=(1, 2))
        z = (score - score.mean()) / score.std()
        prob = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
        m = accumulate(tab, prob[:, None], H, W, 4, 0.5)[0]
        ay, ax = np.unravel_index(int(np.argmax(m)), m.shape)
        assert by <= ay < by + 8 and bx <= ax < bx + 8, (trial, (by, bx), (ay, ax))
        top = _faith_ranks(m)[:64]
        inside = ((top // W >= by) & (top // W < by + 8) & (top % W >= bx) & (top % W < bx + 8)).mean()
        shares.append(float(inside))
    print("share of the 64 top-ranked pixels inside the block:", " ".join(f"{v:.2f}" for v in shares))
    assert min(shares) >= 0.8


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def _lib():
    from sm3hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_entry_points_are_declared_bound_and_exported():
    from sm3hip import _lib as L
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sm3_hip.h")).read(), flags=re.S)
    lib = _lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text)
        assert name in L.SIGNATURES
        assert hasattr(lib, name)
    assert lib.sm3_abi_version() == 9  # additive: the version stays
    from sm3hip import ops, rise
    assert callable(rise.rise) and callable(ops.rise_table) and callable(ops.rise_compose) and callable(ops.rise_accumulate)
    assert ops.RISE_ROW_WORDS == ROW and rise.threshold(0.25) == threshold(0.25) == 2 ** 30
    assert "rise.hip" in open(os.path.join(ROOT, "skin-sm3_amd", "csrc", "Makefile")).read()


def _p(v):
    return C.c_void_p(v) if v else C.c_void_p(0)


def _table(lib, table=0x1000, i0=0, c=4, m=0, H=32, W=32, s=4, p=0.5, seed=1):
    return lib.sm3_rise_table(_p(table), i0, c, m, H, W, s, p, seed, C.c_void_p(0))


def _compose(lib, x=0x1000, base=0x2000, base_n=1, table=0x3000, out=0x4000, N=2, H=32, W=32, s=4, c=4):
    return lib.sm3_rise_compose(_p(x), _p(base), base_n, _p(table), _p(out), N, H, W, s, c, C.c_void_p(0))


def _accumulate(lib, table=0x1000, weights=0x2000, maps=0x3000, sn=8 * 2 * 1024, st=2 * 1024, N=2, T=8, M=4, H=32, W=32, s=4,
                p=0.5):
    return lib.sm3_rise_accumulate(_p(table), _p(weights), _p(maps), sn, st, N, T, M, H, W, s, p, C.c_void_p(0))


@pytest.mark.parametrize("kw,code", [
    (dict(table=0), -1), (dict(i0=-1), -1), (dict(c=0), -1), (dict(i0=2 ** 20 - 3), -1), (dict(c=2 ** 20 + 1), -1),
    (dict(m=2), -1), (dict(m=-1), -1), (dict(H=0), -1), (dict(W=0), -1), (dict(H=2 ** 13, W=2 ** 12), -1), (dict(s=0), -1),
    (dict(s=31, H=64, W=64), -1), (dict(s=33), -1), (dict(H=8, s=9), -1), (dict(W=8, s=9), -1), (dict(p=0.0), -1),
    (dict(p=1.0), -1), (dict(p=-0.5), -1), (dict(p=float("nan")), -1), (dict(p=2.0 ** -33), -1),
    (dict(table=0x1004), -2), (dict(table=0x1008), -2)])
def test_table_rejects_bad_arguments_before_any_launch(kw, code):
    assert _table(_lib(), **kw) == code, kw


@pytest.mark.parametrize("kw,code", [
    (dict(x=0), -1), (dict(base=0), -1), (dict(table=0), -1), (dict(out=0), -1), (dict(N=0), -1), (dict(N=2 ** 16), -1),
    (dict(c=0), -1), (dict(c=8 * 65535 + 1), -1), (dict(base_n=3), -1), (dict(base_n=0), -1), (dict(H=0), -1), (dict(W=-1), -1),
    (dict(H=2 ** 13, W=2 ** 12), -1), (dict(s=0), -1), (dict(s=31, H=64, W=64), -1), (dict(H=8, s=9), -1),
    (dict(H=3, W=5, s=1), -2), (dict(x=0x1004), -2), (dict(base=0x2008), -2), (dict(table=0x3004), -2), (dict(out=0x4008), -2)])
def test_compose_rejects_bad_arguments_before_any_launch(kw, code):
    assert _compose(_lib(), **kw) == code, kw


@pytest.mark.parametrize("kw,code", [
    (dict(table=0), -1), (dict(weights=0), -1), (dict(maps=0), -1), (dict(N=0), -1), (dict(T=0), -1), (dict(M=0), -1),
    (dict(M=2 ** 20 + 1), -1), (dict(sn=-4), -1), (dict(st=-4), -1), (dict(H=0), -1), (dict(H=2 ** 13, W=2 ** 12), -1),
    (dict(s=0), -1), (dict(s=31, H=64, W=64), -1), (dict(W=8, s=9), -1), (dict(p=0.0), -1), (dict(p=1.0), -1),
    (dict(p=float("nan")), -1), (dict(N=2 ** 16, T=2 ** 4), -1),
    (dict(H=3, W=5, s=1), -2), (dict(table=0x1008), -2), (dict(weights=0x2002), -2), (dict(maps=0x3004), -2),
    (dict(sn=8 * 2 * 1024 + 2), -2), (dict(st=2 * 1024 + 1), -2)])
def test_accumulate_rejects_bad_arguments_before_any_launch(kw, code):
    assert _accumulate(_lib(), **kw) == code, kw


# ---- the driver's host logic ------------------------------------------------------------------------------------------------
def test_driver_refuses_bad_arguments_before_touching_a_device():
    from sm3hip.rise import rise
    from src.models.baseline import Baseline
    m = Baseline("resnet18", None)
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(ValueError, match="rise.*eval mode"):
        rise(m.train(), x, x)
    m.eval()
    with pytest.raises(ValueError, match="rise.*CUDA tensor"):
        rise(m, x, x)
    with pytest.raises(TypeError, match="Baseline"):
        rise(torch.nn.Linear(2, 2), x, x)
    for bad in (0, -1, 2 ** 20 + 1, 8.0, True, "8", None):
        with pytest.raises(ValueError, match="rise.*masks"):
            rise(m, x, x, masks=bad)
    for bad in (0, 31, -7, 7.0, True, None):
        with pytest.raises(ValueError, match="rise.*cells"):
            rise(m, x, x, cells=bad)
    with pytest.raises(ValueError, match="rise.*cells must be at most"):
        rise(m, torch.zeros(1, 3, 8, 16), torch.zeros(1, 3, 8, 16), cells=9)
    for bad in (0, 1, 0.0, 1.0, -0.5, 1.5, float("nan"), 2.0 ** -33, True, "0.5", None):
        with pytest.raises(ValueError, match="rise.*p must be"):
            rise(m, x, x, p=bad)
    for bad in (-1, 2 ** 64, 1.0, True, None):
        with pytest.raises(ValueError, match="rise.*seed"):
            rise(m, x, x, seed=bad)
    for bad in (0, 9, -1, 1.5, True):
        with pytest.raises(ValueError, match="rise.*chunk"):
            rise(m, x, x, masks=8, chunk=bad)
    with pytest.raises(ValueError, match="rise.*modality"):
        rise(m, x, x, modality="both")
    with pytest.raises(ValueError, match="rise.*baseline"):
        rise(m, x, x, baseline="black")
    with pytest.raises(ValueError, match="rise.*multiple of 4"):
        rise(m, torch.zeros(1, 3, 3, 5), torch.zeros(1, 3, 3, 5), cells=3)


def test_wrappers_refuse_host_tensors_and_mismatched_shapes():
    from sm3hip import ops
    tab = torch.zeros(4, ROW, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        ops.rise_table(tab, 0, 0, 8, 8, 2, 0.5, 1)
    x, out = torch.zeros(2, 3, 8, 8), torch.zeros(4, 2, 3, 8, 8)
    with pytest.raises(ValueError, match="GPU"):
        ops.rise_compose(x, x[:1], tab, out, 2)
    with pytest.raises(ValueError, match="GPU"):
        ops.rise_accumulate(tab, torch.zeros(4, 16), torch.zeros(2, 8, 8, 8), 2, 0.5)


# ---- the tools ----------------------------------------------------------------------------------------------------------
def _tool(name):
    return _load(f"sm3_{name}_rise_cpu", os.path.join(TOOLS, f"{name}.py"))


SYN = ["--data-path", "-", "--data-name", "synthetic"]


@pytest.mark.parametrize("tool,method", [("backbone_attr", "ig"), ("mlc_attr", "ig"), ("backbone_faith", "cam"),
                                         ("mlc_faith", "cam")])
def test_parsers_take_the_rise_flags(tool, method):
    t = _tool(tool)
    a = t.get_parser().parse_args(SYN)
    assert (a.method, a.rise_masks, a.rise_cells, a.rise_p, a.attr_seed, a.chunk, a.steps, a.samples) == (
        method, 4000, 7, 0.5, 0, None, 32, 16)
    a = t.get_parser().parse_args(SYN + ["--method", "rise", "--rise-masks", "512", "--rise-cells", "5", "--rise-p", "0.25",
                                         "--attr-seed", "11", "--chunk", "64", "--target", "cls", "--max-cases", "3"])
    assert (a.method, a.rise_masks, a.rise_cells, a.rise_p, a.attr_seed, a.chunk, a.target, a.max_cases) == (
        "rise", 512, 5, 0.25, 11, 64, "cls", 3)


@pytest.fixture
def no_gpu(monkeypatch):
    """Anything that reaches for the device fails the test."""
    def boom(*a, **k):
        raise AssertionError("touched the GPU before refusing")
    monkeypatch.setattr(torch, "Generator", boom)
    monkeypatch.setattr(torch.cuda, "synchronize", boom)
    monkeypatch.setattr(torch.nn.Module, "to", boom)
    from sm3hip import attr, cam, faith, rise
    monkeypatch.setattr(attr, "integrated_gradients", boom)
    monkeypatch.setattr(attr, "smooth_grad", boom)
    monkeypatch.setattr(cam, "grad_cam", boom)
    monkeypatch.setattr(faith, "deletion_insertion", boom)
    monkeypatch.setattr(rise, "rise", boom)


RISE_REFUSALS = [
    (["--rise-masks", "0"], "rise-masks"),
    (["--rise-masks", "1048577"], "rise-masks"),
    (["--rise-cells", "0"], "rise-cells"),
    (["--rise-cells", "31"], "rise-cells"),
    (["--rise-p", "0"], "rise-p"),
    (["--rise-p", "1"], "rise-p"),
    (["--attr-seed", "-1"], "attr-seed"),
    (["--attr-seed", str(2 ** 64)], "attr-seed"),
    (["--max-cases", "0"], "max-cases"),
]
ATTR_RISE_REFUSALS = RISE_REFUSALS + [
    (["--rise-masks", "8", "--chunk", "9"], "chunk"),
    (["--chunk", "0"], "chunk"),
    (["--chunk", "4001"], "chunk"),
]
FAITH_RISE_REFUSALS = RISE_REFUSALS + [
    (["--curve-steps", "8", "--chunk", "9"], "chunk"),
    (["--curve-steps", "0"], "curve-steps"),
    (["--modality", "both"], "modality"),
]


@pytest.mark.parametrize("argv,msg", ATTR_RISE_REFUSALS + [(["--img-sz", "16", "16", "--rise-cells", "17"], "rise-cells"),
                                                           (["--img-sz", "3", "5", "--rise-cells", "2"], "multiple of 4")])
def test_backbone_attr_rise_refusals_stop_before_any_kernel(argv, msg, no_gpu, tmp_path):
    with pytest.raises(SystemExit, match=msg):
        _tool("backbone_attr").main(SYN + ["--method", "rise"] + argv + ["--log-path", str(tmp_path)])


@pytest.mark.parametrize("argv,msg", ATTR_RISE_REFUSALS + [(["--test-sz", "16", "--rise-cells", "17"], "rise-cells")])
def test_mlc_attr_rise_refusals_stop_before_any_kernel(argv, msg, no_gpu, tmp_path):
    with pytest.raises(SystemExit, match=msg):
        _tool("mlc_attr").main(SYN + ["--method", "rise"] + argv + ["--log-path", str(tmp_path)])


@pytest.mark.parametrize("argv,msg", FAITH_RISE_REFUSALS + [(["--img-sz", "16", "16", "--rise-cells", "17"], "rise-cells")])
def test_backbone_faith_rise_refusals_stop_before_any_kernel(argv, msg, no_gpu, tmp_path):
    with pytest.raises(SystemExit, match=msg):
        _tool("backbone_faith").main(SYN + ["--method", "rise"] + argv + ["--log-path", str(tmp_path)])


@pytest.mark.parametrize("argv,msg", FAITH_RISE_REFUSALS + [(["--test-sz", "16", "--rise-cells", "17"], "rise-cells")])
def test_mlc_faith_rise_refusals_stop_before_any_kernel(argv, msg, no_gpu, tmp_path):
    with pytest.raises(SystemExit, match=msg):
        _tool("mlc_faith").main(SYN + ["--method", "rise"] + argv + ["--log-path", str(tmp_path)])


@pytest.mark.parametrize("tool", ["backbone_attr", "mlc_attr", "backbone_faith", "mlc_faith"])
def test_occlusion_stays_refused_and_rise_is_named(tool, no_gpu, tmp_path):
    with pytest.raises(SystemExit, match="method.*rise"):
        _tool(tool).main(SYN + ["--method", "occlusion", "--log-path", str(tmp_path)])
