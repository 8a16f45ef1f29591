"""GPU: deletion / insertion faithfulness curves (csrc/faith.hip, sm3hip/faith.py, tools/backbone_faith.py, tools/mlc_faith.py).

  * sm3_faith_rank equal to the numpy restatement of tests/test_faith_cpu.py (integers: exact) on random, heavily tied, constant
    and special-valued maps at sizes from 4 to 448^2 and 1 to 128 rows, and on real Grad-CAM and Integrated-Gradients maps;
    sm3_faith_compose bit-equal to the numpy selection for every window, both directions and any cut into chunks;
  * exact-f32 curves of the ResNet-50 and ResNet-18 Baseline and of the inference.py model (v4 and v2 label projectors) against
    the float64 restatement fed the same ranks, with the torch float32 restatement as yardstick;
  * the end-point identities and the AUC against a host recomputation; equal bits across calls, chunks and batch positions; one
    modality against a joint call whose other baseline is the image itself; the 16-bit modes at 224^2 against exact f32 and the
    f32-maps / bf16-maps / random-control table (printed); no side effects; both tools on synthetic data and a derm7pt-shaped tree."""
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


REF = _load("sm3_faith_ref", os.path.join(ROOT, "tests", "test_faith_cpu.py"))     # ranks, counts, compose, the curves
ATTR = _load("sm3_faith_attr_helpers", os.path.join(ROOT, "tests", "test_attr_cpu.py"))  # baseline18, baseline_fn
CAM = _load("sm3_faith_cam_helpers", os.path.join(ROOT, "tests", "test_cam_gpu.py"))   # models, targets, _v2_forward, _tree


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _device_ranks(maps):
    from sm3hip import ops
    m = torch.from_numpy(np.ascontiguousarray(maps, dtype=np.float32)).to(DEV)
    r = torch.full(m.shape, -1, dtype=torch.int32, device=DEV)
    ops.faith_rank(m, r)
    torch.cuda.synchronize()
    return r.cpu().numpy()


def _check_ranks(maps, tag):
    got = _device_ranks(maps)
    want = REF.ranks(maps)
    assert np.array_equal(got, want), (tag, int((got != want).sum()))
    flat = got.reshape(-1, got.shape[-1])
    assert np.array_equal(np.sort(flat, axis=1), np.broadcast_to(np.arange(flat.shape[1], dtype=np.int32), flat.shape)), tag
    return got


# ---- 1. the kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 128])
@pytest.mark.parametrize("HW", [4, 64, 1028, 64 * 64, 34 * 30, 224 * 224, 448 * 448])
def test_ranks_equal_the_numpy_restatement(HW, rows):
    g = np.random.default_rng(HW * 1000 + rows)
    normal = g.standard_normal((rows, HW)).astype(np.float32)
    _check_ranks(normal, "normal")
    _check_ranks(np.floor(g.random((rows, HW)) * 4).astype(np.float32) / 4 - 0.25, "four values")   # -0.25, 0, 0.25, 0.5
    const = np.full((rows, HW), 0.5, np.float32)
    assert np.array_equal(_check_ranks(const, "constant"), np.broadcast_to(np.arange(HW, dtype=np.int32), (rows, HW)))
    pool = np.float32([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754944e-38, 3e38, -3e38, 3.4028235e38, -3.4028235e38, 1.0,
                       -1.0, 0.5])
    special = pool[g.integers(0, pool.size, (rows, HW))]
    _check_ranks(special, "signed zeros, denormals, large")
    mixed = np.where(g.random((rows, HW)) < 0.3, special, normal)
    a = _check_ranks(mixed, "mixed")
    assert np.array_equal(a, _device_ranks(mixed))                                                    # two calls


def test_ranks_of_a_batched_tensor_with_the_layout_of_the_driver():
    g = np.random.default_rng(5)
    maps = np.round(g.standard_normal((2, 8, 2, 1024)) * 2).astype(np.float32)
    assert np.array_equal(_device_ranks(maps), REF.ranks(maps))


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


def test_ranks_of_real_grad_cam_and_integrated_gradients_maps():
    from sm3hip.attr import integrated_gradients
    from sm3hip.cam import grad_cam
    model, _ = _resnet18(torch.float32)
    derm, clinic = [t.to(DEV) for t in _pair(5)]
    cam = grad_cam(model, derm, clinic)["maps"]
    ig = integrated_gradients(model, derm, clinic, steps=4)["maps"]
    torch.cuda.synchronize()
    c = cam.cpu().numpy().reshape(2, 8, 2, -1)
    live = c.max(axis=-1) > 0
    assert live.any() and (c == 0).sum() > 0 and np.all(c.max(axis=-1)[live] > 0.99)  # exact zeros, and a one per live map
    for name, maps in (("grad_cam", c), ("integrated_gradients", ig.cpu().numpy().reshape(2, 8, 2, -1))):
        got = _check_ranks(maps, name)
        ties = sum(int(np.unique(r).size < r.size) for r in maps.reshape(-1, maps.shape[-1]))
        print(f"{name}: {ties} of {maps.size // maps.shape[-1]} maps hold tied values; top pixel's rank 0 in all: "
              f"{bool(np.all(np.take_along_axis(got, maps.argmax(-1)[..., None], -1) == 0))}")


def _device_compose(x, base, rk, k0, c, steps, invert):
    """rk [N, T, HW] is placed in modality 1 of a [N, T, 2, H, W] tensor, the layout the driver passes."""
    from sm3hip import ops
    N, _, HW = x.shape
    T = rk.shape[1]
    full = torch.full((N, T, 2, 1, HW), -7, dtype=torch.int32)
    full[:, :, 1, 0] = torch.from_numpy(rk)
    full = full.to(DEV)
    out = torch.full((c, T, N, 3, 1, HW), float("nan"), device=DEV)
    ops.faith_compose(torch.from_numpy(x).to(DEV).view(N, 3, 1, HW), torch.from_numpy(base).to(DEV).view(-1, 3, 1, HW),
                      full[:, :, 1], out, k0, steps, invert)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(c, T, N, 3, HW)


@pytest.mark.parametrize("N,T,HW,base_n", [(2, 8, 64 * 64, 1), (3, 8, 1028, 3), (1, 1, 4, 1), (2, 3, 34 * 30, 2), (2, 2, 224 * 224, 1)])
def test_compose_is_the_numpy_selection_bit_for_bit(N, T, HW, base_n):
    g = np.random.default_rng(N * HW + T)
    x = g.standard_normal((N, 3, HW)).astype(np.float32)
    x[0, 0, :4] = np.float32([0.0, -0.0, np.nan, np.inf])                         # bit copies: payloads and signs survive
    base = g.standard_normal((base_n, 3, HW)).astype(np.float32)
    base[0, 1, :2] = np.float32([-0.0, 1e-45])
    rk = np.stack([np.stack([g.permutation(HW) for _ in range(T)]) for _ in range(N)]).astype(np.int32)
    for S in sorted(s for s in {1, 7, 32, HW} if s <= HW):
        windows = [(0, S + 1)] if S <= 32 else [(0, 3), (S - 2, 3), (S // 2, 2)]     # (k0, c): with c_k = 0 and c_k = HW
        for invert in (0, 1):
            for k0, c in windows:
                got = _device_compose(x, base, rk, k0, c, S, invert)
                want = REF.compose(x, base, rk, k0, c, S, invert)
                assert np.array_equal(_bits(got), _bits(want)), (S, invert, k0, c)
            if S <= 32:                                                             # any cut into chunks is the one call
                whole = _device_compose(x, base, rk, 0, S + 1, S, invert)
                for chunk in (1, 4, S + 1):
                    parts = [_device_compose(x, base, rk, k, min(chunk, S + 1 - k), S, invert) for k in range(0, S + 1, chunk)]
                    assert np.array_equal(_bits(np.concatenate(parts)), _bits(whole)), (S, invert, chunk)
                b = np.broadcast_to(base, x.shape)
                first, last = (x, b) if not invert else (b, x)
                assert all(np.array_equal(_bits(whole[0, t]), _bits(first)) for t in range(T))
                assert all(np.array_equal(_bits(whole[S, t]), _bits(last)) for t in range(T))


# ---- 2. the curves against float64 --------------------------------------------------------------------------------------
S, NB, STEPS = 64, 2, 8
# max |engine - fp64| over the probabilities of both curves.  The bound the project holds its other [0, 1]-valued outputs to
# (Grad-CAM maps, tests/test_cam_gpu.py): 1e-3.  The probabilities are continuous in the inputs, so no switched ReLU unit excuses
# a miss.  Measured (engine / torch f32), Grad-CAM maps then IG maps: ResNet-50 Baseline 1.3e-5 / 3.2e-5, 3.3e-5 / 3.9e-5; ResNet-18
# Baseline 1.9e-6 / 9.0e-7, 1.1e-6 / 1.0e-6; v4 Model 8.6e-7 / 3.8e-7, 3.8e-6 / 1.9e-6; v2 Model 2.0e-5 / 6.4e-6, 2.9e-5 / 1.5e-5: 30x
# inside the bound, so it stays.
BOUND = 1e-3


def _oracle_fn(which, state, dt):
    from oracle import sm3_oracle as O
    P, Bf = O.split_state(state, dt, requires_grad=False)
    fwd = {"baseline": O.baseline_forward, "v4": O.inference_forward, "v2": CAM._v2_forward}[which]
    return lambda d, c: fwd(P, Bf, d, c)


def _case(which, dtype):
    """(model on the GPU, fn(dt) -> the restatement's forward in dtype dt)."""
    if which == "resnet18":
        m, cpu = _resnet18(dtype)
        return m, lambda dt: ATTR.baseline_fn(cpu, dt)
    model, state = CAM._model(which, dtype)
    return model, lambda dt: _oracle_fn(which, state, dt)


def _maps(method, model, derm, clinic, tc):
    from sm3hip.attr import integrated_gradients
    from sm3hip.cam import grad_cam
    if method == "cam":
        return grad_cam(model, derm, clinic, target=tc)["maps"]
    return integrated_gradients(model, derm, clinic, target=tc, steps=4)["maps"]


def _host_auc(curve):
    c = curve.double().cpu()
    n = c.shape[-1] - 1
    return (c[..., 0] / 2 + c[..., 1:n].sum(-1) + c[..., n] / 2) / n


def _check_identities(out, steps):
    """The end points against the returned logits bit for bit; the AUCs against a host recomputation from the curves."""
    tc = out["target_class"]
    pick = lambda lg: torch.stack([torch.softmax(o.double(), dim=1).gather(1, tc[:, t:t + 1])[:, 0] for t, o in enumerate(lg)], 1)
    at_x, at_b = pick(out["logits"]), pick(out["baseline_logits"])
    if "deletion" in out:
        assert torch.equal(out["deletion"][..., 0], at_x) and torch.equal(out["deletion"][..., steps], at_b)
    if "insertion" in out:
        assert torch.equal(out["insertion"][..., steps], at_x) and torch.equal(out["insertion"][..., 0], at_b)
    for name in ("deletion", "insertion"):
        if name in out:
            c, a = out[name], out[name + "_auc"]
            assert c.dtype == torch.float64 and a.dtype == torch.float64 and a.shape == c.shape[:2]
            assert float(c.min()) >= 0 and float(c.max()) <= 1
            assert float((a.cpu() - _host_auc(c)).abs().max()) <= 1e-12


@pytest.mark.parametrize("method", ["cam", "ig"])
@pytest.mark.parametrize("which", ["baseline", "resnet18", "v4", "v2"])
def test_exact_f32_curves_against_fp64_on_the_same_ranks(which, method):
    from sm3hip.faith import deletion_insertion
    model, fn = _case(which, torch.float32)
    derm, clinic = _pair(5)
    tc = CAM._targets(7)
    maps = _maps(method, model, derm.to(DEV), clinic.to(DEV), tc.to(DEV))
    out = deletion_insertion(model, derm.to(DEV), clinic.to(DEV), maps, target=tc.to(DEV), steps=STEPS)
    torch.cuda.synchronize()
    del model
    assert out["deletion"].shape == out["insertion"].shape == (NB, 8, STEPS + 1)
    assert out["ranks"].shape == (NB, 8, 2, S, S) and out["ranks"].dtype == torch.int32
    assert torch.equal(out["target_class"].cpu(), tc) and out["steps"] == STEPS and out["modality"] == "joint"
    rk = out["ranks"].cpu()
    assert np.array_equal(rk.numpy(), REF.ranks(maps.cpu().numpy().reshape(NB, 8, 2, -1)).reshape(NB, 8, 2, S, S))
    _check_identities(out, STEPS)
    zero = torch.zeros(1, 3, S, S, dtype=torch.float64)
    ref64 = REF.ref_deletion_insertion(fn(torch.float64), derm.double(), clinic.double(), zero, zero, rk, tc, STEPS)
    ref32 = REF.ref_deletion_insertion(fn(torch.float32), derm, clinic, zero.float(), zero.float(), rk, tc, STEPS)
    diff = lambda a, k: float((a[k].double().cpu() - ref64[k]).abs().max())
    err = max(diff(out, "deletion"), diff(out, "insertion"))
    yard = max(diff(ref32, "deletion"), diff(ref32, "insertion"))
    auc = max(diff(out, "deletion_auc"), diff(out, "insertion_auc"))
    span = float((ref64["deletion"].amax(-1) - ref64["deletion"].amin(-1)).max())
    print(f"{which} {method} maps, {STEPS} curve steps: max |engine - fp64| over the probabilities {err:.3e}; torch f32 {yard:.3e}; "
          f"AUCs {auc:.3e}; largest swing of a deletion curve {span:.3f}; mean deletion / insertion AUC (fp64) "
          f"{float(ref64['deletion_auc'].mean()):.4f} / {float(ref64['insertion_auc'].mean()):.4f}")
    assert err < BOUND, (err, yard)
    assert auc < BOUND, auc


# ---- 3. equal bits -------------------------------------------------------------------------------------------------------
CURVE_KEYS = ("deletion", "insertion", "deletion_auc", "insertion_auc", "ranks", "target_class")


@pytest.mark.parametrize("which", ["baseline", "v4"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_equal_bits_across_calls_chunks_and_batch_positions(which, dtype):
    """Rests on the batch-position and batch-size independence of the eval-mode forward that
    tests/test_cam_gpu.py::test_equal_bits_across_calls_and_batch_positions asserts, here at c * 8 * N images."""
    from sm3hip.cam import grad_cam
    from sm3hip.faith import deletion_insertion
    model, _ = CAM._model(which, dtype)
    derm, clinic = [t.to(DEV) for t in _pair(41, n=2)]
    maps = grad_cam(model, derm, clinic)["maps"]
    steps = 7
    a = deletion_insertion(model, derm, clinic, maps, steps=steps)
    _check_identities(a, steps)
    # the two end points are reused, so a call walks the steps - 1 = 6 interior steps: 3 -> 3 + 3; 4 -> 4 + 2 and 5 -> 5 + 1 end
    # in a shorter last chunk
    for chunk in (steps, 1, 3, 4, 5, None):
        b = deletion_insertion(model, derm, clinic, maps, steps=steps, chunk=chunk)
        for k in CURVE_KEYS:
            assert torch.equal(a[k], b[k]), (chunk, k)
        assert all(torch.equal(p, q) for p, q in zip(a["logits"] + a["baseline_logits"], b["logits"] + b["baseline_logits"]))
    perm = torch.tensor([1, 0], device=DEV)
    c = deletion_insertion(model, derm[perm], clinic[perm], maps[perm], steps=steps, chunk=2)
    for k in CURVE_KEYS:
        assert torch.equal(a[k][perm], c[k]), k
    for mode in ("deletion", "insertion"):
        d = deletion_insertion(model, derm, clinic, maps, steps=steps, mode=mode, chunk=2)
        other = "insertion" if mode == "deletion" else "deletion"
        assert other not in d and other + "_auc" not in d
        assert torch.equal(d[mode], a[mode]) and torch.equal(d[mode + "_auc"], a[mode + "_auc"])
    one = deletion_insertion(model, derm, clinic, maps, steps=1)                    # S = 1: the two end points alone
    assert torch.equal(one["deletion"][..., 0], a["deletion"][..., 0]) and torch.equal(one["deletion"][..., 1], a["deletion"][..., steps])
    assert torch.equal(one["deletion_auc"], one["insertion_auc"])


@pytest.mark.parametrize("which", ["resnet18", "v4"])
def test_one_modality_is_a_joint_call_whose_other_baseline_is_the_image(which):
    from sm3hip.cam import grad_cam
    from sm3hip.faith import deletion_insertion
    model, _ = _case(which, torch.float32)
    derm, clinic = [t.to(DEV) for t in _pair(8)]
    maps = grad_cam(model, derm, clinic)["maps"]
    base = torch.full((1, 3, S, S), 0.25, device=DEV)
    for modality, pair in (("derm", (base, clinic)), ("clinic", (derm, base))):
        a = deletion_insertion(model, derm, clinic, maps, steps=5, baseline=(base, base), modality=modality)
        b = deletion_insertion(model, derm, clinic, maps, steps=5, baseline=pair, modality="joint")
        for k in CURVE_KEYS:
            assert torch.equal(a[k], b[k]), (modality, k)
        assert all(torch.equal(p, q) for p, q in zip(a["baseline_logits"], b["baseline_logits"]))
        assert a["modality"] == modality
        _check_identities(a, 5)
    j = deletion_insertion(model, derm, clinic, maps, steps=5, baseline=(base, base))
    assert not torch.equal(j["deletion"], a["deletion"])
    z = deletion_insertion(model, derm, clinic, maps, steps=5)
    e = deletion_insertion(model, derm, clinic, maps, steps=5, baseline=(torch.zeros(3, S, S), torch.zeros_like(clinic)))
    assert torch.equal(z["deletion"], e["deletion"]) and torch.equal(z["insertion"], e["insertion"])


# ---- 4. the 16-bit modes and the table the metric exists for ---------------------------------------------------------------
def test_16bit_modes_and_16bit_maps_scored_at_224():
    """Recorded, not bounded (asserted: finite and in [0, 1]): what the 16-bit encoders do to the curves of one fixed set of
    ranks, and what 16-bit maps lose when the exact-f32 model scores them, beside the random control.  Measured (procedural
    weights, IG maps of 8 steps, 16 curve steps): bf16 encoders max |p - p_f32| 0.171 deletion / 0.112 insertion, AUC difference
    max 7.8e-2 / 2.5e-2, mean 7.8e-3 / 2.5e-3; f16 1.9e-2 / 1.2e-2, AUC max 5.4e-3 / 2.5e-3, mean 6.7e-4 / 3.0e-4.  Mean deletion /
    insertion AUC under the exact-f32 model: f32 maps 0.5470 / 0.5659, bf16 maps 0.5426 / 0.5618, f16 maps 0.5423 / 0.5641,
    random maps 0.5543 / 0.5632."""
    from sm3hip.attr import integrated_gradients
    from sm3hip.faith import deletion_insertion
    derm, clinic = [t.to(DEV) for t in _pair(31, size=224)]
    tc = CAM._targets(3).to(DEV)
    steps = 16
    models = {name: CAM._baseline(dt, seed=21)[0] for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16),
                                                                     ("f16", torch.float16))}
    maps = {name: integrated_gradients(m, derm, clinic, target=tc, steps=8)["maps"] for name, m in models.items()}
    maps["random"] = torch.rand(maps["f32"].shape, generator=torch.Generator().manual_seed(0)).to(DEV)
    ok = lambda o: all(bool(torch.isfinite(o[k]).all()) and float(o[k].min()) >= 0 and float(o[k].max()) <= 1
                       for k in CURVE_KEYS[:4])
    want = deletion_insertion(models["f32"], derm, clinic, maps["f32"], target=tc, steps=steps)
    assert ok(want)
    for name in ("bf16", "f16"):                                                   # one set of ranks, three arithmetic modes
        got = deletion_insertion(models[name], derm, clinic, maps["f32"], target=tc, steps=steps)
        assert ok(got) and torch.equal(got["ranks"], want["ranks"])
        d = {k: float((got[k] - want[k]).abs().max()) for k in CURVE_KEYS[:4]}
        m = {k: float((got[k] - want[k]).abs().mean()) for k in ("deletion_auc", "insertion_auc")}
        print(f"{name} encoders on the f32 maps' ranks, 224^2, {steps} steps: max |p - p_f32| deletion {d['deletion']:.3e}, insertion "
              f"{d['insertion']:.3e}; AUC max (mean) |difference| deletion {d['deletion_auc']:.3e} ({m['deletion_auc']:.3e}), "
              f"insertion {d['insertion_auc']:.3e} ({m['insertion_auc']:.3e})")
    print("maps scored by the exact-f32 model (mean over 2 pairs x 8 labels): deletion AUC / insertion AUC")
    for name, mp in maps.items():
        got = want if name == "f32" else deletion_insertion(models["f32"], derm, clinic, mp, target=tc, steps=steps)
        assert ok(got)
        print(f"  {name:>6} maps: {float(got['deletion_auc'].mean()):.4f} / {float(got['insertion_auc'].mean()):.4f}")


# ---- 5. no side effects ----------------------------------------------------------------------------------------------------
def test_no_side_effects_on_parameters_buffers_and_gradients():
    from sm3hip.bridge import encoder_engine_for
    from sm3hip.faith import deletion_insertion
    model, _ = CAM._mlc_model("v2", torch.bfloat16)
    derm, clinic = [t.to(DEV) for t in _pair(9)]
    maps = torch.rand(2, 8, 2, S, S, generator=torch.Generator().manual_seed(2)).to(DEV)
    deletion_insertion(model, derm, clinic, maps, steps=2)  # binds the parameters into the engines' flat stores
    for q in model.parameters():
        q.grad = torch.full_like(q, 0.5) if q.dim() == 1 else None
    engs = [encoder_engine_for(b) for b in (model.extractor.derm_backbone, model.extractor.clinic_backbone)]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    grads = {n: (q.grad.clone() if q.grad is not None else None) for n, q in model.named_parameters()}
    flat = [e.store.flat_g.clone() for e in engs]
    kept = (derm.clone(), clinic.clone(), maps.clone())
    deletion_insertion(model, derm, clinic, maps, steps=4, chunk=3, target="cls")
    deletion_insertion(model, derm, clinic, maps, steps=3, modality="clinic", mode="insertion")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(kept, (derm, clinic, maps)))
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    for n, q in model.named_parameters():
        assert (q.grad is None) == (grads[n] is None), n
        if q.grad is not None:
            assert torch.equal(q.grad, grads[n]), n
    for e, f in zip(engs, flat):
        assert e.store.flat_g is not None and torch.equal(e.store.flat_g, f)
    assert torch.is_grad_enabled()  # the call runs under no_grad and restores the caller's mode


# ---- 6. the tools ---------------------------------------------------------------------------------------------------------
def _check_faith(saved, n, steps, method, curves=("deletion", "insertion")):
    for name in ("deletion", "insertion"):
        assert (name in saved) == (name in curves) and (name + "_auc" in saved) == (name in curves)
    for name in curves:
        c, a = saved[name], saved[name + "_auc"]
        assert c.shape == (n, 8, steps + 1) and c.dtype == torch.float64 and a.shape == (n, 8) and a.dtype == torch.float64
        assert torch.isfinite(c).all() and float(c.min()) >= 0 and float(c.max()) <= 1
        assert float((a - _host_auc(c)).abs().max()) <= 1e-12
    for key in ("logits", "baseline_logits"):
        assert len(saved[key]) == 8 and all(l.shape == (n, k) for l, k in zip(saved[key], NUM_CLASSES))
    assert saved["target_class"].shape == (n, 8) and saved["targets"].shape == (n, 8) and saved["indices"].shape == (n,)
    assert saved["method"] == method and len(saved["labels"]) == 8 and "ranks" not in saved and "maps" not in saved


def test_backbone_faith_on_synthetic_data(tmp_path, capsys):
    from src.models.baseline import Baseline
    torch.manual_seed(1)
    path = tmp_path / "best_linear.pth"
    torch.save({"epoch": 1, "state_dict": Baseline("resnet18", None).state_dict()}, path)
    bf = _load("sm3_backbone_faith_gpu", os.path.join(TOOLS, "backbone_faith.py"))
    common = ["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18", "-b", "3", "--img-sz", "64", "64",
              "--max-cases", "5", "--linear-path", str(path), "--curve-steps", "6"]
    stat = bf.main(common + ["--method", "cam", "--chunk", "4", "--log-path", str(tmp_path / "cam")])
    text = capsys.readouterr().out
    assert "images/s" in text and "mean deletion AUC" in text and "mean insertion AUC" in text and stat["images_per_s"] > 0
    assert 0 <= stat["deletion_auc"] <= 1 and 0 <= stat["insertion_auc"] <= 1
    _check_faith(torch.load(tmp_path / "cam" / "faith.pt", map_location="cpu", weights_only=False), 5, 6, "cam")
    bf.main(common + ["--method", "ig", "--steps", "3", "--curve-mode", "deletion", "--log-path", str(tmp_path / "ig")])
    _check_faith(torch.load(tmp_path / "ig" / "faith.pt", map_location="cpu", weights_only=False), 5, 6, "ig", ("deletion",))
    for seed in ("5", "6"):
        bf.main(common + ["--method", "random", "--attr-seed", seed, "--modality", "derm", "--log-path", str(tmp_path / f"r{seed}")])
    a, b = [torch.load(tmp_path / f"r{s}" / "faith.pt", map_location="cpu", weights_only=False) for s in ("5", "6")]
    _check_faith(a, 5, 6, "random")
    assert a["modality"] == "derm" and not torch.equal(a["deletion"], b["deletion"])


def test_backbone_faith_on_a_derm7pt_tree(tmp_path):
    from sm3hip.metrics import CLS_WEIGHTS
    from src.models.baseline import Baseline
    tree = CAM._tree(tmp_path)
    torch.manual_seed(2)
    path = tmp_path / "best_linear.pth"
    torch.save({"epoch": 1, "state_dict": Baseline("resnet18", None).state_dict()}, path)
    bf = _load("sm3_backbone_faith_gpu2", os.path.join(TOOLS, "backbone_faith.py"))
    for method in ("cam", "ig", "random"):
        bf.main(["--data-name", "SevenPCBaseDataset", "--data-path", str(tree), "-j", "4",
                 "--mean", "0.7833", "0.6712", "0.6026", "--std", "0.2139", "0.2472", "0.2571", "-a", "resnet18", "-b", "4",
                 "--img-sz", "64", "64", "--max-cases", "6", "--target", "cls", "--method", method, "--steps", "3",
                 "--curve-steps", "4", "--linear-path", str(path), "--log-path", str(tmp_path / method)])
        saved = torch.load(tmp_path / method / "faith.pt", map_location="cpu", weights_only=False)
        _check_faith(saved, 6, 4, method)
        assert torch.equal(saved["indices"], torch.arange(6))
        assert torch.equal(saved["target_class"], torch.tensor(CLS_WEIGHTS).expand(6, -1))


def test_mlc_faith_on_synthetic_data(tmp_path):
    path = CAM._mlc_checkpoint(tmp_path, "v3")
    mf = _load("sm3_mlc_faith_gpu", os.path.join(TOOLS, "mlc_faith.py"))
    for method, extra in (("cam", ["--cam-layer", "layer3"]), ("ig", ["--steps", "2"]), ("random", [])):
        stat = mf.main(["--data-name", "synthetic", "--data-path", "-", "-b", "3", "--test-sz", "64", "--max-cases", "4",
                        "--mlc-proj", "v3", "--mlc-proj-dim", "64", "--sa-dim-ff", "64", "--method", method, "--curve-steps", "5",
                        "--checkpoint", str(path), "--log-path", str(tmp_path / method), "--amp", "--amp-dtype", "bf16"] + extra)
        assert stat["images_per_s"] > 0
        saved = torch.load(tmp_path / method / "faith.pt", map_location="cpu", weights_only=False)
        _check_faith(saved, 4, 5, method)
        assert saved["mlc_proj"] == "v3"


def test_mlc_faith_on_a_derm7pt_tree(tmp_path):
    tree = CAM._tree(tmp_path)
    path = CAM._mlc_checkpoint(tmp_path, "v4")
    mf = _load("sm3_mlc_faith_gpu2", os.path.join(TOOLS, "mlc_faith.py"))
    for method in ("cam", "ig", "random"):
        mf.main(["--data-name", "SevenPCBaseDataset", "--data-path", str(tree), "-j", "4", "-b", "4", "--test-sz", "64",
                 "--max-cases", "6", "--mlc-proj", "v4", "--mlc-proj-dim", "64", "--sa-dim-ff", "64", "--method", method,
                 "--steps", "2", "--curve-steps", "4", "--checkpoint", str(path), "--log-path", str(tmp_path / method)])
        saved = torch.load(tmp_path / method / "faith.pt", map_location="cpu", weights_only=False)
        _check_faith(saved, 6, 4, method)
        assert torch.equal(saved["indices"], torch.arange(6))
