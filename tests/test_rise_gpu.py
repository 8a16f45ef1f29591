"""GPU: RISE saliency maps (csrc/rise.hip, sm3hip/rise.py, the four attribution / faithfulness tools with --method rise).

  * sm3_rise_table, sm3_rise_compose and sm3_rise_accumulate equal to the numpy restatement of tests/test_rise_cpu.py with ==
    on the bits, at sizes from 4 x 4 to 448^2, grids of 1 to 30 cells, special values in the images and the weights, any cut
    into chunks;
  * exact-f32 scores of the ResNet-50 and ResNet-18 Baseline and of the inference.py model (v4 and v2 label projectors)
    against the float64 restatement fed the same masks, with the torch float32 restatement as yardstick; the maps bit-equal to
    the numpy accumulation of the engine's own scores, and inside the bound that follows against the float64 maps;
  * equal bits across calls, chunks, batch positions and batch sizes; one modality against a joint call whose other baseline
    is the image itself; the 16-bit modes at 224^2 against exact f32 and the RISE / IG / Grad-CAM / random faithfulness table
    (printed); no side effects; the four tools on synthetic data and a derm7pt-shaped tree."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
DEV = "cuda:0"
NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REF = _load("sm3_rise_ref", os.path.join(ROOT, "tests", "test_rise_cpu.py"))            # table, masks, compose, accumulate
ATTR = _load("sm3_rise_attr_helpers", os.path.join(ROOT, "tests", "test_attr_cpu.py"))  # baseline18, baseline_fn
CAM = _load("sm3_rise_cam_helpers", os.path.join(ROOT, "tests", "test_cam_gpu.py"))     # models, targets, _v2_forward, _tree


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the kernels -----------------------------------------------------------------------------------------------------
def _device_table(seed, m, i0, c, H, W, s, p):
    from sm3hip import ops
    t = torch.full((c, REF.ROW), -1, dtype=torch.int32, device=DEV)
    ops.rise_table(t, i0, m, H, W, s, p, seed)
    torch.cuda.synchronize()
    return t


SIZES = [(4, 4), (30, 34), (64, 64), (64, 96), (224, 224), (448, 448)]
GEOMETRY = [(H, W, s) for H, W in SIZES for s in (1, 4, 7, 14, 30) if s <= min(H, W)]


@pytest.mark.parametrize("H,W,s", GEOMETRY)
def test_table_equals_the_numpy_restatement(H, W, s):
    for p, seed, m, i0, c in ((0.5, 2 ** 32 + 5, 0, 0, 70), (0.1, 2 ** 63 + 11, 1, 1000, 33), (0.9, 7, 1, 2 ** 20 - 3, 3)):
        got = _device_table(seed, m, i0, c, H, W, s, p).cpu().numpy().view(np.uint32)
        want = REF.table(seed, m, i0, c, H, W, s, p)
        assert np.array_equal(got, want), (p, seed, m, i0)
        parts = [_device_table(seed, m, i0 + k, min(8, c - k), H, W, s, p).cpu().numpy().view(np.uint32) for k in range(0, c, 8)]
        assert np.array_equal(np.concatenate(parts), want)                            # any cut of [i0, i0 + c) is the one call
    share = np.mean([REF.grid_bits(r, s).mean() for r in REF.table(2 ** 32 + 5, 0, 0, 70, H, W, s, 0.1)])
    assert share < 0.3                                                                # p reaches the bits


def test_wrappers_refuse_what_the_kernels_do_not_take():
    from sm3hip import ops
    tab = torch.zeros(4, REF.ROW, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="table"):
        ops.rise_table(torch.zeros(4, 32, dtype=torch.int32, device=DEV), 0, 0, 8, 8, 2, 0.5, 1)
    with pytest.raises(ValueError, match="seed"):
        ops.rise_table(tab, 0, 0, 8, 8, 2, 0.5, -1)
    x = torch.zeros(2, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="do not match"):
        ops.rise_compose(x, x[:1], tab, torch.zeros(3, 2, 3, 8, 8, device=DEV), 2)
    with pytest.raises(ValueError, match="weights"):
        ops.rise_accumulate(tab, torch.zeros(4, 15, device=DEV), torch.zeros(2, 8, 8, 8, device=DEV), 2, 0.5)
    with pytest.raises(ValueError, match="contiguous"):
        ops.rise_accumulate(tab, torch.zeros(4, 16, device=DEV), torch.zeros(2, 8, 8, 16, device=DEV)[..., ::2], 2, 0.5)


def _images(g, N, H, W, base_n):
    x = g.standard_normal((N, 3, H, W)).astype(np.float32)
    x[0, 0].reshape(-1)[:4] = np.float32([-0.0, np.nan, np.inf, -np.inf])
    x[N - 1, 2].reshape(-1)[-4:] = np.float32([np.inf, -0.0, 1e-45, np.nan])
    base = g.standard_normal((base_n, 3, H, W)).astype(np.float32)
    base[0, 1].reshape(-1)[:4] = np.float32([-0.0, 1e-45, 0.0, np.inf])
    return x, base


def _device_compose(x, base, tab, s):
    from sm3hip import ops
    N, _, H, W = x.shape
    out = torch.full((tab.shape[0], N, 3, H, W), float("nan"), device=DEV)
    ops.rise_compose(torch.from_numpy(x).to(DEV), torch.from_numpy(base).to(DEV), tab, out, s)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bits(got, want, x):
    """Equal bits, a NaN that x itself holds included (it is passed on, payload and sign, by all three operations).  Only where
    an operation MAKES a NaN (inf - inf, 0 * inf: the restatement holds a NaN and x does not) must the device just hold a NaN:
    IEEE 754 leaves the sign and the payload of such a NaN to the implementation, and the host and the device choose differently
    (the host's default NaN has the sign bit set)."""
    g, w = _bits(got), _bits(want)
    made = np.isnan(want) & ~np.broadcast_to(np.isnan(x), want.shape)
    return bool(np.isnan(got[made]).all() and np.array_equal(g[~made], w[~made]))


@pytest.mark.parametrize("H,W,s,N,base_n", [(4, 4, 1, 1, 1), (4, 4, 4, 3, 3), (30, 34, 7, 2, 1), (30, 34, 30, 3, 1), (64, 64, 7, 2, 2),
                                            (64, 96, 14, 3, 1), (64, 64, 1, 2, 1), (224, 224, 7, 2, 1), (224, 224, 30, 1, 1),
                                            (448, 448, 14, 1, 1)])
def test_compose_equals_the_numpy_restatement(H, W, s, N, base_n):
    g = np.random.default_rng(H * W + s + N)
    x, base = _images(g, N, H, W, base_n)
    c = 11 if H < 448 else 3
    for p in (0.1, 0.5, 0.9):
        tab = _device_table(2 ** 33 + 9, 1, 5, c, H, W, s, p)
        rows = tab.cpu().numpy().view(np.uint32)
        got = _device_compose(x, base, tab, s)
        want = REF.compose(x, base, rows, H, W, s)
        assert got.shape == want.shape == (c, N, 3, H, W) and _same_bits(got, want, x), p
        for chunk in (1, 4):                                                          # any cut into chunks is the one call
            parts = [_device_compose(x, base, tab[k:k + chunk], s) for k in range(0, c, chunk)]
            assert np.array_equal(_bits(np.concatenate(parts)), _bits(got)), (p, chunk)
    # hand-made tables: all corners set keeps x through the three operations, none gives base + 0 * (x - base)
    hand = np.stack([REF._hand_row(s, range((s + 2) ** 2), 0, 0), REF._hand_row(s, [], 0, 0)])
    got = _device_compose(x, base, torch.from_numpy(hand.view(np.int32)).to(DEV), s)
    assert _same_bits(got, REF.compose(x, base, hand, H, W, s), x)
    b = np.broadcast_to(base, x.shape)
    fin = np.isfinite(x) & np.isfinite(b)
    with np.errstate(all="ignore"):
        assert np.array_equal(got[1][fin], (b + np.float32(0) * (x - b))[fin])


def _weights(g, M, R):
    w = g.random((M, R)).astype(np.float32)
    pool = np.float32([0.0, 1.0, 1e-45, 1e-40, 1.1754944e-38, 0.5])
    pick = g.random((M, R)) < 0.3
    w[pick] = pool[g.integers(0, pool.size, int(pick.sum()))]
    return w


def _device_accumulate(tab, w, N, T, H, W, s, p):
    """The output goes to modality 1 of a [N, T, 2, H, W] tensor, the layout the driver passes; modality 0 stays untouched."""
    from sm3hip import ops
    maps = torch.full((N, T, 2, H, W), -7.0, device=DEV)
    ops.rise_accumulate(tab, torch.from_numpy(w).to(DEV), maps[:, :, 1], s, p)
    torch.cuda.synchronize()
    assert bool((maps[:, :, 0] == -7.0).all())
    return maps[:, :, 1].cpu().numpy()


@pytest.mark.parametrize("H,W,s", [(4, 4, 1), (30, 34, 7), (64, 64, 7), (64, 96, 30), (224, 224, 7), (448, 448, 14)])
@pytest.mark.parametrize("M,N,T", [(1, 1, 1), (5, 1, 8), (64, 8, 8), (257, 3, 8)])
def test_accumulate_equals_the_numpy_restatement(H, W, s, M, N, T):
    g = np.random.default_rng(H + W + s + M + N * T)
    p = (0.1, 0.5, 0.9)[(M + H) % 3]
    tab = _device_table(2 ** 35 + 1, 0, 0, M, H, W, s, p)
    w = _weights(g, M, N * T)
    want = REF.accumulate(tab.cpu().numpy().view(np.uint32), w, H, W, s, p).reshape(N, T, H, W)
    got = _device_accumulate(tab, w, N, T, H, W, s, p)
    assert np.array_equal(_bits(got), _bits(want))


# ---- 2. end to end in exact f32 against float64 -------------------------------------------------------------------------
S, NB, MASKS, CELLS, P = 64, 2, 48, 7, 0.5
# max |engine - fp64| over the scores (probabilities).  The bound the project holds its other [0, 1]-valued outputs to (Grad-CAM
# maps, tests/test_cam_gpu.py; the faithfulness curves, tests/test_faith_gpu.py): 1e-3.  Measured (engine / torch f32): ResNet-50
# Baseline 4.6e-5 / 3.6e-5, ResNet-18 Baseline 1.8e-6 / 1.1e-6, v4 Model 4.6e-5 / 9.4e-6, v2 Model 2.2e-5 / 1.1e-5: 21x inside the
# bound, so it stays.  max |maps - fp64 maps| 5.3e-6 / 4.5e-7 / 3.2e-6 / 1.4e-6 against derived bounds of 9.8e-5 / 1.0e-5 / 9.7e-5 /
# 4.9e-5.
BOUND = 1e-3


def _resnet18(dtype, seed=13):
    cpu = ATTR.baseline18(seed)
    m = copy.deepcopy(cpu)
    for b in (m.derm_backbone, m.clinic_backbone):
        b.sm3_dtype = dtype
    return m.to(DEV).eval(), cpu


def _pair(seed, size=64, n=2):
    from oracle import procedural
    derm, clinic = procedural.make_pair_batch(n, size, seed)
    return torch.from_numpy(derm[0]), torch.from_numpy(clinic[0])


def _oracle_fn(which, state, dt):
    from oracle import sm3_oracle as O
    Pm, Bf = O.split_state(state, dt, requires_grad=False)
    fwd = {"baseline": O.baseline_forward, "v4": O.inference_forward, "v2": CAM._v2_forward}[which]
    return lambda d, c: fwd(Pm, Bf, d, c)


def _case(which, dtype):
    """(model on the GPU, fn(dt) -> the restatement's forward in dtype dt)."""
    if which == "resnet18":
        m, cpu = _resnet18(dtype)
        return m, lambda dt: ATTR.baseline_fn(cpu, dt)
    model, state = CAM._model(which, dtype)
    return model, lambda dt: _oracle_fn(which, state, dt)


def ref_scores(fn, derm, clinic, masks, tc, modality="joint", group=8):
    """[N, 8, M] float64 probabilities softmax(logits_t.double())[tc] at the masked pairs, computed in the dtype of the images:
    the masked inputs are mask * x (zero baseline); masks [2, M, H, W] in that dtype; `group` masks per forward (eval-mode rows
    are independent)."""
    N, M = derm.shape[0], masks.shape[1]
    out = torch.empty(N, 8, M, dtype=torch.float64)
    put = lambda x, mk, on: (x[None] * mk[:, None, None] if on else x[None].expand(mk.shape[0], -1, -1, -1, -1)).reshape(
        (-1,) + tuple(x.shape[1:]))
    with torch.no_grad():
        for i0 in range(0, M, group):
            n = min(group, M - i0)
            d = put(derm, masks[0, i0:i0 + n], modality in ("joint", "derm"))
            c = put(clinic, masks[1, i0:i0 + n], modality in ("joint", "clinic"))
            for t, lg in enumerate(fn(d, c)):
                pr = torch.softmax(lg.double(), dim=1).gather(1, tc[:, t].repeat(n)[:, None]).view(n, N)
                out[:, t, i0:i0 + n] = pr.t()
    return out


def _numpy_maps(out, seed, H, W, modalities=(0, 1)):
    """The numpy accumulation of the engine's own scores: [N, 8, 2, H, W]."""
    N, M = out["scores"].shape[0], out["masks"]
    w = out["scores"].permute(2, 0, 1).reshape(M, N * 8).float().cpu().numpy()
    maps = np.zeros((N, 8, 2, H, W), np.float32)
    for m in modalities:
        tab = REF.table(seed, m, 0, M, H, W, out["cells"], out["p"])
        maps[:, :, m] = REF.accumulate(tab, w, H, W, out["cells"], out["p"]).reshape(N, 8, H, W)
    return maps


@pytest.mark.parametrize("which", ["baseline", "resnet18", "v4", "v2"])
def test_exact_f32_scores_and_maps_against_fp64_on_the_same_masks(which):
    from sm3hip.rise import rise
    model, fn = _case(which, torch.float32)
    derm, clinic = _pair(5)
    tc = CAM._targets(7)
    seed = 2 ** 34 + 17
    out = rise(model, derm.to(DEV), clinic.to(DEV), target=tc.to(DEV), masks=MASKS, cells=CELLS, p=P, seed=seed)
    torch.cuda.synchronize()
    del model
    assert out["maps"].shape == (NB, 8, 2, S, S) and out["maps"].dtype == torch.float32
    assert out["scores"].shape == (NB, 8, MASKS) and out["scores"].dtype == torch.float64
    assert torch.equal(out["target_class"].cpu(), tc) and len(out["logits"]) == 8
    assert (out["masks"], out["cells"], out["p"], out["seed"], out["modality"]) == (MASKS, CELLS, P, seed, "joint")
    assert 1 <= out["chunk"] <= MASKS
    masks = np.stack([REF.masks_of(REF.table(seed, m, 0, MASKS, S, S, CELLS, P), S, S, CELLS) for m in range(2)])
    ref64 = ref_scores(fn(torch.float64), derm.double(), clinic.double(), torch.from_numpy(masks).double(), tc)
    ref32 = ref_scores(fn(torch.float32), derm, clinic, torch.from_numpy(masks), tc)
    got = out["scores"].cpu()
    err, yard = float((got - ref64).abs().max()), float((ref32 - ref64).abs().max())
    # the maps: bit-equal to the numpy accumulation of the engine's own scores ...
    maps = out["maps"].cpu().numpy()
    assert np.array_equal(_bits(maps), _bits(_numpy_maps(out, seed, S, S)))
    # ... hence |maps - maps_fp64| <= max |dP| / p (every mask value is at most 1: M terms of |dP| over M p) + the rounding of the
    # M products, M sums, the weights and the division: M 2^-23 max(maps)
    maps64 = torch.einsum("nti,mihw->ntmhw", ref64, torch.from_numpy(masks).double()) / (MASKS * P)
    merr = float((torch.from_numpy(maps).double() - maps64).abs().max())
    mbound = err / P + MASKS * 2.0 ** -23 * float(maps.max())
    swing = float((ref64.amax(-1) - ref64.amin(-1)).max())
    print(f"{which}, {MASKS} masks: max |scores - fp64| {err:.3e}; torch f32 {yard:.3e}; largest swing of a score over the masks "
          f"{swing:.3f}; max |maps - fp64 maps| {merr:.3e} (bound {mbound:.3e}); maps in [{maps.min():.4f}, {maps.max():.4f}]")
    assert err < BOUND, (err, yard)
    assert merr <= mbound, (merr, mbound)


# ---- 3. equal bits -------------------------------------------------------------------------------------------------------
KEYS = ("maps", "scores", "target_class")


def _equal(a, b, keys=KEYS):
    return all(torch.equal(a[k], b[k]) for k in keys) and all(torch.equal(p, q) for p, q in zip(a["logits"], b["logits"]))


@pytest.mark.parametrize("which", ["baseline", "v4"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_equal_bits_across_calls_chunks_batch_positions_and_batch_sizes(which, dtype):
    """Rests on the batch-position and batch-size independence of the eval-mode forward that
    tests/test_cam_gpu.py::test_equal_bits_across_calls_and_batch_positions asserts, here at c * N images."""
    from sm3hip.rise import rise
    model, _ = CAM._model(which, dtype)
    derm, clinic = [t.to(DEV) for t in _pair(41, n=2)]
    kw = dict(masks=MASKS, cells=5, p=0.25, seed=2 ** 40 + 1)
    a = rise(model, derm, clinic, **kw)
    assert bool(torch.isfinite(a["maps"]).all()) and float(a["maps"].min()) >= 0
    for chunk in (None, 1, 5, 7, 48):
        b = rise(model, derm, clinic, chunk=chunk, **kw)
        assert _equal(a, b), chunk
        assert b["chunk"] == (chunk or b["chunk"])
    perm = torch.tensor([1, 0], device=DEV)
    c = rise(model, derm[perm], clinic[perm], chunk=7, **kw)                          # the other batch position
    assert all(torch.equal(a[k][perm], c[k]) for k in KEYS)
    tc = a["target_class"]
    for n in (0, 1):                                                                  # a batch of one
        d = rise(model, derm[n:n + 1], clinic[n:n + 1], target=tc[n:n + 1], chunk=5, **kw)
        assert all(torch.equal(a[k][n:n + 1], d[k]) for k in KEYS), n
    e = rise(model, derm, clinic, **dict(kw, seed=kw["seed"] + 1))
    assert not torch.equal(a["scores"], e["scores"]) and not torch.equal(a["maps"], e["maps"])
    t0 = _device_table(kw["seed"], 0, 0, 4, S, S, 5, 0.25)
    assert not torch.equal(t0, _device_table(kw["seed"] + 1, 0, 0, 4, S, S, 5, 0.25))  # different seeds, different masks
    assert not torch.equal(t0, _device_table(kw["seed"], 1, 0, 4, S, S, 5, 0.25))      # and the two modalities' masks differ


@pytest.mark.parametrize("which", ["resnet18", "v4"])
def test_one_modality_is_a_joint_call_whose_other_baseline_is_the_image(which):
    from sm3hip.rise import rise
    model, _ = _case(which, torch.float32)
    derm, clinic = [t.to(DEV) for t in _pair(8)]
    base = torch.full((1, 3, S, S), 0.25, device=DEV)
    kw = dict(masks=24, cells=4, p=0.5, seed=3)
    for modality, m, pair in (("derm", 0, (base, clinic)), ("clinic", 1, (derm, base))):
        a = rise(model, derm, clinic, baseline=(base, base), modality=modality, **kw)
        b = rise(model, derm, clinic, baseline=pair, modality="joint", **kw)
        assert torch.equal(a["scores"], b["scores"]) and torch.equal(a["maps"][:, :, m], b["maps"][:, :, m]), modality
        assert not bool(a["maps"][:, :, 1 - m].any()) and a["modality"] == modality   # the unperturbed modality: zeros
        assert bool(a["maps"][:, :, m].any())
    j = rise(model, derm, clinic, baseline=(base, base), **kw)
    assert not torch.equal(j["scores"], a["scores"])
    z = rise(model, derm, clinic, **kw)
    e = rise(model, derm, clinic, baseline=(torch.zeros(3, S, S), torch.zeros_like(clinic)), **kw)
    assert _equal(z, e)


# ---- 4. no side effects ----------------------------------------------------------------------------------------------------
def test_no_side_effects_on_parameters_buffers_and_gradients():
    from sm3hip.bridge import encoder_engine_for
    from sm3hip.rise import rise
    model, _ = CAM._mlc_model("v2", torch.bfloat16)
    derm, clinic = [t.to(DEV) for t in _pair(9)]
    rise(model, derm, clinic, masks=4)  # binds the parameters into the engines' flat stores
    for q in model.parameters():
        q.grad = torch.full_like(q, 0.5) if q.dim() == 1 else None
    engs = [encoder_engine_for(b) for b in (model.extractor.derm_backbone, model.extractor.clinic_backbone)]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    grads = {n: (q.grad.clone() if q.grad is not None else None) for n, q in model.named_parameters()}
    flat = [e.store.flat_g.clone() for e in engs]
    kept = (derm.clone(), clinic.clone())
    rise(model, derm, clinic, masks=12, chunk=5, target="cls")
    rise(model, derm, clinic, masks=6, modality="clinic", cells=3, p=0.3)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(kept, (derm, clinic)))
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    for n, q in model.named_parameters():
        assert (q.grad is None) == (grads[n] is None), n
        if q.grad is not None:
            assert torch.equal(q.grad, grads[n]), n
    for e, f in zip(engs, flat):
        assert e.store.flat_g is not None and torch.equal(e.store.flat_g, f)
    assert torch.is_grad_enabled()  # the call runs under no_grad and restores the caller's mode


# ---- 5. the 16-bit modes and the table the feature exists for --------------------------------------------------------------
def _pearson(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / (a.norm() * b.norm() + 1e-30))


def test_16bit_modes_against_exact_f32_at_224():
    """Recorded, not bounded: nobody has measured what the 16-bit encoders do to a RISE map.  Asserted: finite, non-negative
    and at most (1 + M 2^-23) max(scores) / p, the sum's own bound (every mask value is at most 1).  Measured
    (maps up to 1.106): bf16 max |map - map_f32| 5.6e-2, mean 5.4e-3, Pearson per map mean 0.8105; f16 6.4e-3, 5.9e-4, 0.8125 =
    26 / 32 -- 6 of the 32 maps give Pearson 0.0000 in both modes (maps without variance), the other 26 average 0.9975 / 1.0000."""
    from sm3hip.rise import rise
    derm, clinic = [t.to(DEV) for t in _pair(31, size=224)]
    tc = CAM._targets(3).to(DEV)
    M = 256
    outs = {}
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16), ("f16", torch.float16)):
        model = CAM._baseline(dt, seed=21)[0]
        outs[name] = o = rise(model, derm, clinic, target=tc, masks=M, seed=5)
        del model
        mp = o["maps"]
        assert bool(torch.isfinite(mp).all()) and float(mp.min()) >= 0
        assert float(mp.max()) <= (1 + M * 2.0 ** -23) * float(o["scores"].max()) / 0.5
    want = outs["f32"]["maps"]
    for name in ("bf16", "f16"):
        got = outs[name]["maps"]
        d = (got - want).abs()
        r = [_pearson(got[n, t, m], want[n, t, m]) for n in range(2) for t in range(8) for m in range(2)]
        ds = (outs[name]["scores"] - outs["f32"]["scores"]).abs()
        print(f"{name} encoders, 224^2, {M} masks: max (mean) |map - map_f32| {float(d.max()):.3e} ({float(d.mean()):.3e}), maps up to "
              f"{float(want.max()):.3f}; Pearson per map min {min(r):.4f} mean {np.mean(r):.4f}; max (mean) |score - score_f32| "
              f"{float(ds.max()):.3e} ({float(ds.mean()):.3e})")


def test_faithfulness_of_rise_beside_ig_grad_cam_and_random_at_224():
    """The table the feature exists for, printed, asserted only finite and in [0, 1]: ResNet-50 Baseline with
    procedural weights, 224^2, 2 pairs, 16 curve steps; RISE (512 masks), IG (8 steps), Grad-CAM and uniform random maps, in exact
    f32 and in bf16 (maps made and scored by the same model).  Measured, mean deletion / insertion AUC: f32 RISE 0.5012 / 0.6148,
    IG 0.5470 / 0.5659, Grad-CAM 0.5202 / 0.5824, random 0.5543 / 0.5632; bf16 RISE 0.5038 / 0.6146, IG 0.5485 / 0.5640, Grad-CAM
    0.5206 / 0.5828, random 0.5582 / 0.5671."""
    from sm3hip.attr import integrated_gradients
    from sm3hip.cam import grad_cam
    from sm3hip.faith import deletion_insertion
    from sm3hip.rise import rise
    derm, clinic = [t.to(DEV) for t in _pair(31, size=224)]
    tc = CAM._targets(3).to(DEV)
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        model = CAM._baseline(dt, seed=21)[0]
        maps = {"rise": rise(model, derm, clinic, target=tc, masks=512, seed=1)["maps"],
                "ig": integrated_gradients(model, derm, clinic, target=tc, steps=8)["maps"],
                "cam": grad_cam(model, derm, clinic, target=tc)["maps"],
                "random": torch.rand(2, 8, 2, 224, 224, generator=torch.Generator().manual_seed(0)).to(DEV)}
        print(f"{name} model, mean over 2 pairs x 8 labels: deletion AUC / insertion AUC")
        for method, mp in maps.items():
            got = deletion_insertion(model, derm, clinic, mp, target=tc, steps=16)
            for k in ("deletion", "insertion", "deletion_auc", "insertion_auc"):
                assert bool(torch.isfinite(got[k]).all()) and float(got[k].min()) >= 0 and float(got[k].max()) <= 1
            print(f"  {method:>6} maps: {float(got['deletion_auc'].mean()):.4f} / {float(got['insertion_auc'].mean()):.4f}")
        del model


# ---- 6. the tools ---------------------------------------------------------------------------------------------------------
def _read(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def _check_attr(saved, n, size, M):
    assert saved["maps"].shape == (n, 8, 2, size, size) and saved["maps"].dtype == torch.float16
    assert saved["scores"].shape == (n, 8, M) and saved["scores"].dtype == torch.float64
    assert float(saved["scores"].min()) >= 0 and float(saved["scores"].max()) <= 1
    assert bool(torch.isfinite(saved["maps"].float()).all()) and float(saved["maps"].float().min()) >= 0
    assert len(saved["logits"]) == 8 and all(l.shape == (n, c) for l, c in zip(saved["logits"], NUM_CLASSES))
    assert saved["target_class"].shape == (n, 8) and saved["targets"].shape == (n, 8) and saved["indices"].shape == (n,)
    assert saved["method"] == "rise" and "delta" not in saved


def _check_faith(saved, n, size, steps):
    for name in ("deletion", "insertion"):
        c, a = saved[name], saved[name + "_auc"]
        assert c.shape == (n, 8, steps + 1) and c.dtype == torch.float64 and a.shape == (n, 8)
        assert torch.isfinite(c).all() and float(c.min()) >= 0 and float(c.max()) <= 1
    assert saved["maps"].shape == (n, 8, 2, size, size) and saved["maps"].dtype == torch.float16
    assert saved["method"] == "rise" and saved["target_class"].shape == (n, 8)


RISE_FLAGS = ["--method", "rise", "--rise-masks", "20", "--rise-cells", "4", "--rise-p", "0.4", "--attr-seed", "9"]


def test_backbone_tools_on_synthetic_data(tmp_path, capsys):
    from src.models.baseline import Baseline
    torch.manual_seed(1)
    path = tmp_path / "best_linear.pth"
    torch.save({"epoch": 1, "state_dict": Baseline("resnet18", None).state_dict()}, path)
    ba = _load("sm3_backbone_attr_rise_gpu", os.path.join(TOOLS, "backbone_attr.py"))
    bf = _load("sm3_backbone_faith_rise_gpu", os.path.join(TOOLS, "backbone_faith.py"))
    common = ["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "-b", "3", "--img-sz", "64", "64",
              "--max-cases", "5", "--linear-path", str(path)] + RISE_FLAGS
    stat = ba.main(common + ["--log-path", str(tmp_path / "a")])
    text = capsys.readouterr().out
    assert "rise" in text and "20 masks" in text and "images/s" in text and stat["images_per_s"] > 0
    a = _read(tmp_path / "a" / "attr.pt")
    _check_attr(a, 5, 64, 20)
    for chunk in ("1", "7", "20"):                                                   # --chunk: masks per forward, the same bits
        ba.main(common + ["--chunk", chunk, "--log-path", str(tmp_path / f"a{chunk}")])
        b = _read(tmp_path / f"a{chunk}" / "attr.pt")
        assert torch.equal(a["maps"], b["maps"]) and torch.equal(a["scores"], b["scores"]), chunk
    stat = bf.main(common + ["--curve-steps", "6", "--chunk", "4", "--log-path", str(tmp_path / "f")])
    assert 0 <= stat["deletion_auc"] <= 1 and 0 <= stat["insertion_auc"] <= 1
    f = _read(tmp_path / "f" / "faith.pt")
    _check_faith(f, 5, 64, 6)
    assert torch.equal(f["maps"], a["maps"])                                         # the faith tool scores the attr tool's maps
    bf.main(common + ["--curve-steps", "6", "--modality", "derm", "--log-path", str(tmp_path / "fd")])
    d = _read(tmp_path / "fd" / "faith.pt")
    assert d["modality"] == "derm" and not bool(d["maps"][:, :, 1].any()) and bool(d["maps"][:, :, 0].any())


def test_backbone_tools_on_a_derm7pt_tree(tmp_path):
    from sm3hip.metrics import CLS_WEIGHTS
    from src.models.baseline import Baseline
    tree = CAM._tree(tmp_path)
    torch.manual_seed(2)
    path = tmp_path / "best_linear.pth"
    torch.save({"epoch": 1, "state_dict": Baseline("resnet18", None).state_dict()}, path)
    common = ["--data-name", "SevenPCBaseDataset", "--data-path", str(tree), "-j", "4", "--mean", "0.7833", "0.6712", "0.6026",
              "--std", "0.2139", "0.2472", "0.2571", "-a", "resnet18", "-b", "4", "--img-sz", "64", "64", "--max-cases", "6",
              "--target", "cls", "--linear-path", str(path)] + RISE_FLAGS
    ba = _load("sm3_backbone_attr_rise_gpu2", os.path.join(TOOLS, "backbone_attr.py"))
    bf = _load("sm3_backbone_faith_rise_gpu2", os.path.join(TOOLS, "backbone_faith.py"))
    ba.main(common + ["--log-path", str(tmp_path / "a")])
    bf.main(common + ["--curve-steps", "4", "--log-path", str(tmp_path / "f")])
    a, f = _read(tmp_path / "a" / "attr.pt"), _read(tmp_path / "f" / "faith.pt")
    _check_attr(a, 6, 64, 20)
    _check_faith(f, 6, 64, 4)
    assert torch.equal(a["maps"], f["maps"]) and torch.equal(a["indices"], torch.arange(6))
    assert torch.equal(a["target_class"], torch.tensor(CLS_WEIGHTS).expand(6, -1))
    # the masks are the same for every case: a case's map does not depend on its batch
    ba.main(common + ["-b", "2", "--chunk", "3", "--log-path", str(tmp_path / "a2")])
    assert torch.equal(_read(tmp_path / "a2" / "attr.pt")["maps"], a["maps"])


def test_mlc_tools_on_synthetic_data(tmp_path):
    path = CAM._mlc_checkpoint(tmp_path, "v3")
    common = ["--data-name", "synthetic", "--data-path", "-", "-b", "3", "--test-sz", "64", "--max-cases", "4", "--mlc-proj", "v3",
              "--mlc-proj-dim", "64", "--sa-dim-ff", "64", "--checkpoint", str(path), "--amp", "--amp-dtype", "bf16"] + RISE_FLAGS
    ma = _load("sm3_mlc_attr_rise_gpu", os.path.join(TOOLS, "mlc_attr.py"))
    mf = _load("sm3_mlc_faith_rise_gpu", os.path.join(TOOLS, "mlc_faith.py"))
    stat = ma.main(common + ["--log-path", str(tmp_path / "a")])
    assert stat["images_per_s"] > 0
    a = _read(tmp_path / "a" / "attr.pt")
    _check_attr(a, 4, 64, 20)
    ma.main(common + ["--chunk", "6", "--log-path", str(tmp_path / "a6")])
    assert torch.equal(_read(tmp_path / "a6" / "attr.pt")["maps"], a["maps"])
    mf.main(common + ["--curve-steps", "5", "--log-path", str(tmp_path / "f")])
    f = _read(tmp_path / "f" / "faith.pt")
    _check_faith(f, 4, 64, 5)
    assert torch.equal(f["maps"], a["maps"]) and f["mlc_proj"] == "v3"


def test_mlc_tools_on_a_derm7pt_tree(tmp_path):
    tree = CAM._tree(tmp_path)
    path = CAM._mlc_checkpoint(tmp_path, "v4")
    common = ["--data-name", "SevenPCBaseDataset", "--data-path", str(tree), "-j", "4", "-b", "4", "--test-sz", "64",
              "--max-cases", "6", "--mlc-proj", "v4", "--mlc-proj-dim", "64", "--sa-dim-ff", "64", "--checkpoint", str(path)] + \
        RISE_FLAGS
    ma = _load("sm3_mlc_attr_rise_gpu2", os.path.join(TOOLS, "mlc_attr.py"))
    mf = _load("sm3_mlc_faith_rise_gpu2", os.path.join(TOOLS, "mlc_faith.py"))
    ma.main(common + ["--log-path", str(tmp_path / "a")])
    mf.main(common + ["--curve-steps", "4", "--log-path", str(tmp_path / "f")])
    a, f = _read(tmp_path / "a" / "attr.pt"), _read(tmp_path / "f" / "faith.pt")
    _check_attr(a, 6, 64, 20)
    _check_faith(f, 6, 64, 4)
    assert torch.equal(a["maps"], f["maps"]) and torch.equal(a["indices"], torch.arange(6))
