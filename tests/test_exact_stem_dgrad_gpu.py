"""Bit-exact checks of the stem data gradient (sm3_stem_dgrad_bn, csrc/stem.hip: stem_dgrad_kernel) at its tile edges and
across the tiles of a persistent workgroup.

The operands are those of the stem weight-gradient table (exact_inputs.stem_wgrad_case): dz, xo and the filter are small
integers, the BatchNorm operands are dyadic and the count is a power of two, so dxo = A dz - B xo + C is exact in fp32 and
representable in every storage type, every product of the GEMM is exact and every partial sum stays below 2^24 quanta
(test_stem_dgrad_preconditions asserts this on the CPU for the whole table).  Whatever the tiling, the K order or the grid,
dx must then equal fp64 torch.nn.grad.conv2d_input of the fp64 dxo: no tolerance, +0 and -0 identified.

One tile is 16 row pairs by 64 column pairs (one image), a wave covers 16 column pairs, and the grid is min(tiles, 512) in
the 16-bit modes and min(tiles, 256) in exact f32.  The table holds a single pixel, images below the 7-tap support, a full
tile with and without the last parity row and column, one row pair and one column pair past both tile edges (halos across
both seams), and two geometries with more tiles than any grid: there a workgroup restages its LDS ring and its output tile
under a finished tile and reloads the BatchNorm coefficients when its next tile belongs to the other view.

dx is a slice of a sentinel-filled buffer whose surroundings must come back unchanged; the inputs must come back
unchanged; a refused call writes nothing.  The binding passes gamma=None through as a null pointer (the kernel reads it as
1), so the frozen-statistics test runs both forms.
"""
import ctypes
import functools
import time

import pytest
import torch

from exact_inputs import Guarded, _dev, draw, need_exact, need_repr, quantum, same, stem_wgrad_case

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
IDS = ["f32", "bf16", "f16"]
LAUNCHES = [0]

# N, H, W, BatchNorm views
DGRAD_GEOMS = [
    (1, 1, 1, 1),       # one pixel, centre tap only
    (2, 2, 3, 2),       # below the filter support, two views of one image each
    (1, 5, 8, 1),       # H below 7
    (3, 13, 7, 1),      # W at 7, odd
    (4, 10, 12, 2),     # small, two images per view
    (1, 31, 127, 1),    # Ho = 16, Wo = 64, odd: a full tile whose last parity row and column do not exist
    (2, 32, 128, 2),    # exact tile fit
    (1, 33, 129, 1),    # 2 x 2 tiles; the tail tiles own one row pair / one column pair without their r = 1 / q = 1 half
    (2, 34, 130, 2),    # the same seams with the parity half present
    (1040, 2, 2, 2),    # 1040 tiles: 2 to 5 per workgroup; tile 512 is view 0, tile 1024 is view 1
    (258, 33, 3, 2),    # 516 tiles of two row chunks: workgroups go from a view-0 tile to a view-1 tile with a multi-row ring
]


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def tiles_of(N, H, W):
    Ho, Wo = out_hw(H, W)
    return N * ((Ho + 15) // 16) * ((Wo + 63) // 64)


def dxo_ref(c, N, H, W, views, frozen=False, gamma=True):
    """fp64 dxo = gamma * invstd[v] * (dz - gs0 / count - xhat * gs1 / count) per view, as [N, 64, Ho, Wo]."""
    Ho, Wo = out_hw(H, W)
    M = N * Ho * Wo
    v = torch.arange(M) // (M // views)
    gs = torch.zeros_like(c["gs"]) if frozen else c["gs"]
    g = c["gamma"] if gamma else torch.ones_like(c["gamma"])
    xh = (c["xo"] - c["mean"][v]) * c["invstd"][v]
    dxo = g * c["invstd"][v] * (c["dz"] - gs[v, :64] / c["count"] - xh * gs[v, 64:] / c["count"])
    return dxo.reshape(N, Ho, Wo, 64).permute(0, 3, 1, 2)


def dx_ref(w, dxo, N, H, W):
    return torch.nn.grad.conv2d_input((N, 3, H, W), w, dxo, stride=2, padding=3)


FORMS = {"train": (False, True), "frozen": (True, True), "frozen gamma=None": (True, False)}  # name: (frozen, gamma)


@functools.lru_cache(maxsize=None)
def dgrad_case(dt, i):
    """Case i of the table, built once per type: the operands of stem_wgrad_case (seed 1700 + i) and a filter (seed
    1800 + i)."""
    N, H, W, views = DGRAD_GEOMS[i]
    c = stem_wgrad_case(dt, N, H, W, views, 1700 + i)
    w = draw(torch.Generator().manual_seed(1800 + i), (64, 3, 7, 7), 2, 0.5, 0)
    need_repr(w, dt, "stem dgrad w")
    return dict(c, w=w)


@functools.lru_cache(maxsize=None)
def dgrad_ref(dt, i, form):
    """The fp64 dx of case i in one form of FORMS, its preconditions asserted; built once and shared, never modified."""
    N, H, W, views = DGRAD_GEOMS[i]
    c = dgrad_case(dt, i)
    dxo = dxo_ref(c, N, H, W, views, *FORMS[form])
    need_repr(dxo, dt, f"stem dgrad dxo ({form})")
    need_exact(dx_ref(c["w"].abs(), dxo.abs(), N, H, W), quantum(c["w"]) * quantum(dxo), f"stem dgrad sum ({form})")
    return dx_ref(c["w"], dxo, N, H, W)


def test_stem_dgrad_preconditions():
    """CPU self-check: every case of the table, in every type and form, satisfies the exactness preconditions it is run
    under; the table reaches what it claims to reach and the references are not trivially zero."""
    for i, (N, H, W, views) in enumerate(DGRAD_GEOMS):
        for dt in DTYPES:
            refs = {form: dgrad_ref(dt, i, form) for form in FORMS}
        ref = refs["train"]
        if ref.numel() > 100:
            assert float((ref != 0).double().mean()) > 0.99, (N, H, W)
        assert bool((ref != 0).any()), (N, H, W)
        assert not torch.equal(ref, refs["frozen"]) and not torch.equal(refs["frozen"], refs["frozen gamma=None"])
    # both multi-tile geometries exceed both grids, and a workgroup's consecutive tiles change view in both
    for N, H, W, views in DGRAD_GEOMS[-2:]:
        tiles = tiles_of(N, H, W)
        assert tiles > 512
        per_image = tiles // N
        view_of = lambda t: (t // per_image) // (N // views)  # noqa: E731
        for grid in (256, 512):
            assert any(view_of(t) != view_of(t + grid) for t in range(tiles - grid)), (N, H, W, grid)
    assert [tiles_of(*g[:3]) for g in DGRAD_GEOMS[5:9]] == [1, 2, 4, 8]


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
def _g(t, dt):
    return t.to(dt).to(_dev()).contiguous()


def ops():
    from sm3hip import ops as o
    return o


def device_operands(c, dt, frozen=False):
    gs = torch.zeros_like(c["gs"]) if frozen else c["gs"]
    return dict(dz=_g(c["dz"], dt), xo=_g(c["xo"], dt), mean=_g(c["mean"], F32), invstd=_g(c["invstd"], F32),
                gamma=_g(c["gamma"], F32), gs=_g(gs, torch.float64), count=c["count"],
                w=_g(c["w"].permute(0, 2, 3, 1).reshape(64, 147), F32))  # the fp32 master, [co][kh][kw][c]


def run(d, dt, N, H, W, views, gamma=True):
    """One launch into a guarded dx; the guards and the inputs are checked here."""
    o = ops()
    keep = {k: d[k].clone() for k in ("dz", "xo", "w")}
    dx = Guarded(N * 3 * H * W, F32)
    LAUNCHES[0] += 1
    o.stem_dgrad_bn(o.dtype_code(dt), d["dz"], d["xo"], d["mean"], d["invstd"], d["gamma"] if gamma else None, d["gs"],
                    d["count"], d["w"], dx.t.view(N, 3, H, W), views=views)
    torch.cuda.synchronize()
    tag = f"stem dgrad N{N} H{H} W{W} v{views} {dt}"
    assert dx.guards(), tag + ": wrote outside dx"
    for k, t in keep.items():
        assert torch.equal(d[k], t), tag + f": {k} was modified"
    return dx, tag


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_stem_dgrad_train_mode_bit_exact(dt):
    """Train mode (nonzero global sums), views 1 and 2: dx equal to fp64 over the whole table."""
    LAUNCHES[0] = 0
    t0 = time.perf_counter()
    for i, (N, H, W, views) in enumerate(DGRAD_GEOMS):
        c = dgrad_case(dt, i)
        dx, tag = run(device_operands(c, dt), dt, N, H, W, views)
        same(dx.t, dgrad_ref(dt, i, "train"), tag + " train dx")
    print(f"stem dgrad train {dt}: {LAUNCHES[0]} launches checked in {time.perf_counter() - t0:.2f} s")
    assert LAUNCHES[0] == len(DGRAD_GEOMS)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_stem_dgrad_frozen_and_gamma_none_bit_exact(dt):
    """Frozen statistics (global sums 0), with gamma and with gamma=None (read as 1): dx equal to fp64 over the whole table."""
    LAUNCHES[0] = 0
    t0 = time.perf_counter()
    for i, (N, H, W, views) in enumerate(DGRAD_GEOMS):
        c = dgrad_case(dt, i)
        d = device_operands(c, dt, frozen=True)
        for nm, gamma in (("frozen", True), ("frozen gamma=None", False)):
            dx, tag = run(d, dt, N, H, W, views, gamma=gamma)
            same(dx.t, dgrad_ref(dt, i, nm), f"{tag} {nm} dx")
    print(f"stem dgrad frozen {dt}: {LAUNCHES[0]} launches checked in {time.perf_counter() - t0:.2f} s")
    assert LAUNCHES[0] == 2 * len(DGRAD_GEOMS)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_stem_dgrad_grid_independence(dt):
    """Real (non-dyadic) inputs, where a summation order would show: an image of the 516-tile launch has the bits of the
    same image computed alone (one or two tiles, views = 1) with its view's statistics."""
    N, H, W, views = 258, 33, 3, 2
    Ho, Wo = out_hw(H, W)
    per, M = Ho * Wo, N * Ho * Wo
    g = torch.Generator().manual_seed(1900)
    c = dict(dz=torch.randn(M, 64, generator=g), xo=torch.randn(M, 64, generator=g) * 2 + 0.5,
             w=torch.randn(64, 3, 7, 7, generator=g) * 0.1, mean=torch.randn(views, 64, generator=g) * 0.3 + 0.5,
             invstd=torch.rand(views, 64, generator=g) + 0.25, gamma=torch.randn(64, generator=g),
             gs=torch.randn(views, 128, generator=g).double() * 50, count=float(M // views))
    d = device_operands(c, dt)
    LAUNCHES[0] = 0
    big, tag = run(d, dt, N, H, W, views)
    big = big.t.view(N, 3, H, W)
    assert bool(torch.isfinite(big).all()) and bool((big != 0).any())
    for n in (0, N // views - 1, N // views, N - 1):
        v = n // (N // views)
        one = dict(d, dz=d["dz"][n * per:(n + 1) * per].clone(), xo=d["xo"][n * per:(n + 1) * per].clone(),
                   mean=d["mean"][v].clone(), invstd=d["invstd"][v].clone(), gs=d["gs"][v].clone())
        alone, _ = run(one, dt, 1, H, W, 1)
        assert torch.equal(alone.t.view(torch.int32), big[n].reshape(-1).view(torch.int32)), \
            f"{tag}: image {n} (view {v}) differs from the same image computed alone"
    print(f"stem dgrad grid independence {dt}: {LAUNCHES[0]} launches checked")


@pytest.mark.gpu
def test_stem_dgrad_rejections_leave_dx_untouched():
    """N % views, count = 0, a dz pointer off 16-byte alignment and an unknown dtype code are refused with the codes of
    test_input_grad_cpu.py, through ops where the wrapper lets the call through and through the library handle otherwise;
    dx and everything around it stay untouched."""
    from sm3hip import _lib
    o, L = ops(), _lib.load()
    N, H, W = 4, 10, 12
    c = dgrad_case(BF16, 4)
    d = device_operands(c, BF16)
    code = o.dtype_code(BF16)
    n = d["dz"].numel()
    off = torch.zeros(n + 8, dtype=BF16, device=_dev())[4:4 + n]  # contiguous, 8 bytes off a 16-byte boundary
    assert off.data_ptr() % 16 == 8 and off.is_contiguous()
    dx = Guarded(N * 3 * H * W, F32)
    dxv = dx.t.view(N, 3, H, W)
    args = lambda **k: [dict(d, **k)[x] for x in ("dz", "xo", "mean", "invstd", "gamma", "gs", "count", "w")]  # noqa: E731
    with pytest.raises(_lib.SM3LibraryError, match="SM3_EINVAL"):
        o.stem_dgrad_bn(code, *args(count=0.0), dxv, views=2)
    with pytest.raises(_lib.SM3LibraryError, match="SM3_EALIGN"):
        o.stem_dgrad_bn(code, *args(dz=off), dxv, views=2)
    with pytest.raises(ValueError):  # the wrapper's own refusal
        o.stem_dgrad_bn(code, *args(), dxv, views=3)

    P = lambda t, add=0: ctypes.c_void_p(t.data_ptr() + add)  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(dtype=code, dz_off=0, count=1024.0, views=2):
        return L.sm3_stem_dgrad_bn(dtype, P(d["dz"], dz_off), P(d["xo"]), P(d["mean"]), P(d["invstd"]), P(d["gamma"]),
                                   P(d["gs"]), count, P(d["w"]), P(dx.t), N, H, W, views, st)
    assert raw(views=3) == -1
    assert raw(count=0.0) == -1
    assert raw(dz_off=8) == -2
    assert raw(dtype=7) == -3
    torch.cuda.synchronize()
    assert dx.untouched(), "a refused sm3_stem_dgrad_bn call wrote to dx or around it"
    # the same arguments, accepted: the refusals above were not refusals of something else
    assert raw() == 0
    torch.cuda.synchronize()
    same(dx.t, dgrad_ref(BF16, 4, "train"), "accepted call after the refusals")
    assert dx.guards()
