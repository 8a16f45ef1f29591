"""CPU: Integrated Gradients and SmoothGrad (sm3hip/attr.py, csrc/attr.hip) -- the entry points in the header, the binding and
the library and their host-side refusals; the numpy restatements of the kernels (Philox4x32-10 against its published
known-answer vectors, the normals, alpha_k, the blend) that tests/test_attr_gpu.py compares the device against bit for bit; the
torch restatement of both methods (any dtype: float64 is the reference, float32 the yardstick) against a hand-computable linear
model; the quadrature gap of the restatement at 4 and 64 steps on the model the GPU convergence test uses; the chunk planner;
the two tools' parsers and refusals (each before anything touches the GPU)."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
NUM_CLASSES = [5, 3, 2, 3, 3, 3, 3, 2]
ENTRY_POINTS = ("sm3_attr_path", "sm3_attr_noise", "sm3_attr_accumulate", "sm3_attr_finish")


# ---- numpy restatements of the kernels (used by tests/test_attr_gpu.py) --------------------------------------------------
def alpha_k(k, steps):
    """Midpoint rule, as the kernel computes it: (float)(2k + 1) / (float)(2 * steps), one correctly rounded f32 division."""
    return np.float32(2 * k + 1) / np.float32(2 * steps)


def path_points(x, base, k0, c, steps):
    """sm3_attr_path: out[j] = base + alpha * (x - base), three separately rounded f32 operations.  x [N, E], base [1 | N, E]."""
    x, base = x.astype(np.float32), np.broadcast_to(base.astype(np.float32), x.shape)
    out = np.empty((c,) + x.shape, np.float32)
    for j in range(c):
        d = (x - base).astype(np.float32)
        out[j] = (base + (alpha_k(k0 + j, steps) * d).astype(np.float32)).astype(np.float32)
    return out


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC 2011).  ctr: 4 arrays of uint32 (equal shapes), key: 2 uint32 -> 4 arrays of uint32."""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    c = [np.asarray(v, dtype=np.uint64) for v in ctr]
    k0, k1 = int(key[0]), int(key[1])
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def normals(seed, sample, N, E):
    """z [N, E] of sm3_attr_noise for one sample index: counter (e / 4, n, sample, 0), key = the seed's low and high words;
    Box-Muller in float64 on (w0, w1) and (w2, w3) with u = (w + 0.5) * 2^-32, rounded to f32; element e takes lane e % 4."""
    e4, n = np.meshgrid(np.arange(E // 4, dtype=np.uint32), np.arange(N, dtype=np.uint32))
    w = philox4x32_10([e4, n, np.full_like(e4, sample), np.zeros_like(e4)], (seed & 0xFFFFFFFF, seed >> 32))
    u = [(v.astype(np.float64) + 0.5) * 2.0 ** -32 for v in w]
    z = np.empty((N, E // 4, 4), np.float32)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[a]))
        z[:, :, a] = (r * np.cos(2.0 * np.pi * u[a + 1])).astype(np.float32)
        z[:, :, a + 1] = (r * np.sin(2.0 * np.pi * u[a + 1])).astype(np.float32)
    return z.reshape(N, E)


def accumulate(acc, g, w, squared):
    """sm3_attr_accumulate: acc [N, E] f32, g [c, N, E] f32; every product and sum rounded to f32 on its own, ascending j."""
    acc, w = acc.astype(np.float32).copy(), np.float32(w)
    for j in range(g.shape[0]):
        f = (g[j] * g[j]).astype(np.float32) if squared else g[j].astype(np.float32)
        acc = (acc + (w * f).astype(np.float32)).astype(np.float32)
    return acc


def finish(acc, x, base, mode):
    """sm3_attr_finish: acc [T, N, C, HW] -> (attr, maps [T, N, HW], sums [T, N] float64).  The float64 sum is exact, hence
    order-free, on the small-integer inputs the GPU test feeds it."""
    if mode == 0:
        attr = ((x - np.broadcast_to(base, x.shape)).astype(np.float32)[None] * acc).astype(np.float32)
    else:
        attr = acc.astype(np.float32)
    maps = np.zeros(attr.shape[:2] + attr.shape[3:], np.float32)
    for ch in range(attr.shape[2]):
        maps = (maps + np.abs(attr[:, :, ch])).astype(np.float32)
    return attr, maps, attr.astype(np.float64).sum(axis=(2, 3))


# ---- the torch restatement of the two methods (float64: the reference; float32: the yardstick) ---------------------------
def _label_grads(fn, xs, tc):
    """d logit_t[tc] / d xs for t < 8 at the image batches xs = [derm, clinic] ([M, 3, H, W], leaves); tc [M, 8]."""
    logits = fn(xs[0], xs[1])
    out = []
    for t in range(len(NUM_CLASSES)):
        y = logits[t].gather(1, tc[:, t:t + 1]).sum()  # eval mode: each logit depends on its own sample only
        out.append(torch.autograd.grad(y, xs, retain_graph=t + 1 < len(NUM_CLASSES)))
    return out


def _picked(logits, tc):
    return torch.stack([o.detach().gather(1, tc[:, t:t + 1])[:, 0] for t, o in enumerate(logits)], dim=1)


def ref_integrated_gradients(fn, derm, clinic, base_d, base_c, tc, steps):
    """IG by the midpoint rule in the dtype of the inputs.  fn(derm, clinic) -> 8 logits [M, n_i]; the path is joint over both
    images; all steps go through fn as one batch (eval mode: rows are independent).  Returns attributions [N, 8, 2, 3, H, W],
    logits, baseline_logits and delta [N, 8] = sum(attributions) - (logit_t(x) - logit_t(base))."""
    N, dt = derm.shape[0], derm.dtype
    al = torch.tensor([(2 * k + 1) / (2 * steps) for k in range(steps)], dtype=dt).view(steps, 1, 1, 1, 1)
    xs, bs = [derm, clinic], [base_d.expand_as(derm), base_c.expand_as(clinic)]
    pts = [(b + al * (x - b)).reshape((steps * N,) + x.shape[1:]).detach().requires_grad_() for x, b in zip(xs, bs)]
    grads = _label_grads(fn, pts, tc.repeat(steps, 1))
    attr = torch.stack([torch.stack([(x - b) * (g[m].view((steps, N) + x.shape[1:]).sum(0) / steps)
                                     for m, (x, b) in enumerate(zip(xs, bs))], dim=1) for g in grads], dim=1)
    with torch.no_grad():
        logits, base_logits = fn(derm, clinic), fn(bs[0], bs[1])
    delta = attr.double().sum(dim=(2, 3, 4, 5)) - (_picked(logits, tc).double() - _picked(base_logits, tc).double())
    return {"attributions": attr, "logits": logits, "baseline_logits": base_logits, "delta": delta}


def ref_smooth_grad(fn, noisy_d, noisy_c, tc, squared=False):
    """SmoothGrad from given noisy inputs [S, N, 3, H, W]: the mean over S of the input gradient (or its square)."""
    S, N = noisy_d.shape[:2]
    pts = [x.reshape((S * N,) + x.shape[2:]).detach().requires_grad_() for x in (noisy_d, noisy_c)]
    grads = _label_grads(fn, pts, tc.repeat(S, 1))
    f = (lambda g: g * g) if squared else (lambda g: g)
    return torch.stack([torch.stack([f(g[m]).view((S, N) + pts[m].shape[1:]).sum(0) / S for m in range(2)], dim=1)
                        for g in grads], dim=1)


def resnet_features(m, x):
    """Eval-mode forward of a torchvision-layout ResNet from its own modules' tensors, in the dtype of x."""
    dt = x.dtype
    bn = lambda y, b: F.batch_norm(y, b.running_mean.to(dt), b.running_var.to(dt), b.weight.to(dt), b.bias.to(dt), False, 0.0,
                                   b.eps)
    conv = lambda y, c: F.conv2d(y, c.weight.to(dt), None, c.stride, c.padding, c.dilation, c.groups)
    y = F.max_pool2d(F.relu(bn(conv(x, m.conv1), m.bn1)), 3, 2, 1)
    for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
        for blk in layer:
            idn = y
            out = F.relu(bn(conv(y, blk.conv1), blk.bn1))
            if hasattr(blk, "conv3"):
                out = F.relu(bn(conv(out, blk.conv2), blk.bn2))
                out = bn(conv(out, blk.conv3), blk.bn3)
            else:
                out = bn(conv(out, blk.conv2), blk.bn2)
            if blk.downsample is not None:
                idn = bn(conv(y, blk.downsample[0]), blk.downsample[1])
            y = F.relu(out + idn)
    return y.mean(dim=(2, 3))


def baseline_fn(model, dt):
    """fn(derm, clinic) of a CPU Baseline (any BASELINE_ARCHS architecture) in dtype dt."""
    def fn(derm, clinic):
        feats = torch.cat([resnet_features(model.derm_backbone, derm), resnet_features(model.clinic_backbone, clinic)], dim=1)
        return [F.linear(feats, c.weight.to(dt), c.bias.to(dt)) for c in model.classifier]
    return fn


def baseline18(seed):
    """A ResNet-18 Baseline with non-trivial frozen statistics and heads large enough for O(1) logits (CPU, eval)."""
    from src.models.baseline import Baseline
    torch.manual_seed(seed)
    m = Baseline("resnet18", None)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.1, 0.1)
                mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.1, 0.1)
        for c in m.classifier:
            c.weight.normal_(0.0, 0.05)
            c.bias.normal_(0.0, 0.1)
    return m.eval()


CONV_SEED, CONV_SIZE = 6, 64  # the convergence case of tests/test_attr_gpu.py (chosen here, on the CPU)


def convergence_case():
    from oracle import procedural
    derm, clinic = [torch.from_numpy(a[0]) for a in procedural.make_pair_batch(2, CONV_SIZE, CONV_SEED)]
    g = torch.Generator().manual_seed(CONV_SEED)
    tc = torch.stack([torch.randint(0, n, (2,), generator=g) for n in NUM_CLASSES], dim=1)
    return baseline18(CONV_SEED), derm, clinic, tc


# ---- the restatements against what can be computed by hand ---------------------------------------------------------------
def test_philox4x32_10_known_answers():
    """The known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10([np.array([v], np.uint32) for v in ctr], key)
        assert tuple(int(v[0]) for v in got) == want, [hex(int(v[0])) for v in got]


def test_normals_are_standard_and_a_function_of_seed_sample_position_alone():
    z = normals(7, 3, 4, 4096)
    assert z.dtype == np.float32 and np.isfinite(z).all()
    assert abs(float(z.mean())) < 0.03 and abs(float(z.std()) - 1) < 0.03
    assert np.array_equal(z[:2, :64], normals(7, 3, 2, 64))  # neither the batch nor the row length enters
    assert not np.array_equal(z, normals(7, 4, 4, 4096)) and not np.array_equal(z, normals(8, 3, 4, 4096))
    assert not np.array_equal(z, normals(7 + (1 << 32), 3, 4, 4096))  # the high word of the seed is part of the key


def test_alpha_is_the_midpoint_rule():
    for steps in (1, 3, 8, 32, 50):
        a = np.array([alpha_k(k, steps) for k in range(steps)], np.float64)
        assert np.allclose(a, (np.arange(steps) + 0.5) / steps, rtol=6e-8, atol=0)
        assert abs(a.mean() - 0.5) < 1e-7
    assert alpha_k(0, 1) == np.float32(0.5) and alpha_k(3, 8) == np.float32(0.4375)
    x, b = np.array([[1.0, -2.0, 0.5, 3.0]], np.float32), np.array([[0.0, 2.0, 0.5, -1.0]], np.float32)
    assert np.array_equal(path_points(x, b, 3, 1, 8)[0], np.float32([[0.4375, 0.25, 0.5, 0.75]]))


def _linear_fn(ws):
    return lambda d, c: [torch.einsum("nchw,kchw->nk", d, w[0]) + torch.einsum("nchw,kchw->nk", c, w[1]) + 0.25 for w in ws]


def test_integrated_gradients_of_a_linear_model_is_exact_at_one_step():
    g = torch.Generator().manual_seed(0)
    ws = [(torch.randn(n, 3, 4, 4, generator=g, dtype=torch.float64), torch.randn(n, 3, 4, 4, generator=g, dtype=torch.float64))
          for n in NUM_CLASSES]
    derm, clinic = torch.randn(2, 3, 4, 4, generator=g, dtype=torch.float64), torch.randn(2, 3, 4, 4, generator=g, dtype=torch.float64)
    bd, bc = torch.randn(1, 3, 4, 4, generator=g, dtype=torch.float64), torch.zeros(1, 3, 4, 4, dtype=torch.float64)
    tc = torch.stack([torch.randint(0, n, (2,), generator=g) for n in NUM_CLASSES], dim=1)
    for steps in (1, 5):
        out = ref_integrated_gradients(_linear_fn(ws), derm, clinic, bd, bc, tc, steps)
        assert out["attributions"].shape == (2, 8, 2, 3, 4, 4)
        for t in range(8):
            for n in range(2):
                assert torch.allclose(out["attributions"][n, t, 0], (derm[n] - bd[0]) * ws[t][0][tc[n, t]], rtol=1e-12, atol=1e-13)
                assert torch.allclose(out["attributions"][n, t, 1], clinic[n] * ws[t][1][tc[n, t]], rtol=1e-12, atol=1e-13)
        assert float(out["delta"].abs().max()) < 1e-12  # completeness: exact for a linear model


def test_smooth_grad_restatement_on_a_quadratic_model():
    """logit = sum(w * x^2) / 2: the gradient is w * x, its mean over noisy copies w * mean(x_k); squared: w^2 mean(x_k^2)."""
    g = torch.Generator().manual_seed(1)
    w = torch.randn(3, 4, 4, generator=g, dtype=torch.float64)
    fn = lambda d, c: [((d * d * w).sum((1, 2, 3)) / 2 + (c * w).sum((1, 2, 3)))[:, None].expand(-1, n) for n in NUM_CLASSES]
    nd, nc = torch.randn(5, 2, 3, 4, 4, generator=g, dtype=torch.float64), torch.randn(5, 2, 3, 4, 4, generator=g, dtype=torch.float64)
    tc = torch.zeros(2, 8, dtype=torch.long)
    a = ref_smooth_grad(fn, nd, nc, tc)
    assert a.shape == (2, 8, 2, 3, 4, 4)
    assert torch.allclose(a[:, 3, 0], w * nd.mean(0)) and torch.allclose(a[:, 3, 1], w.expand(2, -1, -1, -1))
    sq = ref_smooth_grad(fn, nd, nc, tc, squared=True)
    assert torch.allclose(sq[:, 0, 0], w * w * (nd * nd).mean(0)) and torch.allclose(sq[:, 0, 1], (w * w).expand(2, -1, -1, -1))


def test_restatement_on_the_oracle_encoder_equals_a_step_by_step_loop():
    """On the oracle's ResNet-50 Baseline (the forward tests/test_cam_cpu.py's ref_grad_cam runs): sending all path points through
    the model as one batch gives what one forward and backward per path point and label gives (eval mode: rows independent)."""
    from oracle import procedural, sm3_oracle as O
    state = procedural.make_state_dict(procedural.baseline_spec(), seed=3)
    P, Bf = O.split_state(state, torch.float64, requires_grad=False)
    derm, clinic = [torch.from_numpy(a[0][:1]).double() for a in procedural.make_pair_batch(2, 64, 3)]
    tc = torch.tensor([[1, 0, 1, 2, 0, 1, 2, 0]])
    fn = lambda d, c: O.baseline_forward(P, Bf, d, c)
    base_d, zero = 0.25 * torch.ones(1, 3, 64, 64, dtype=torch.float64), torch.zeros(1, 3, 64, 64, dtype=torch.float64)
    steps = 2
    out = ref_integrated_gradients(fn, derm, clinic, base_d, zero, tc, steps)
    assert out["attributions"].shape == (1, 8, 2, 3, 64, 64) and out["delta"].shape == (1, 8)
    for t in (0, 5):
        acc = [torch.zeros_like(derm), torch.zeros_like(clinic)]
        for k in range(steps):
            a = (k + 0.5) / steps
            xd, xc = (base_d + a * (derm - base_d)).requires_grad_(), (a * clinic).requires_grad_()
            g = torch.autograd.grad(fn(xd, xc)[t][0, tc[0, t]], [xd, xc])
            acc = [acc[0] + g[0] / steps, acc[1] + g[1] / steps]
        assert torch.allclose(out["attributions"][:, t, 0], (derm - base_d) * acc[0], rtol=1e-9, atol=1e-15)
        assert torch.allclose(out["attributions"][:, t, 1], clinic * acc[1], rtol=1e-9, atol=1e-15)
        gap = out["attributions"][0, t].sum() - (fn(derm, clinic)[t][0, tc[0, t]] - fn(base_d, zero)[t][0, tc[0, t]])
        assert abs(float(gap - out["delta"][0, t])) < 1e-10


def test_accumulate_and_finish_restatements_by_hand():
    g = np.float32([[[1, -2, 3, 0]], [[2, 2, -1, 4]]])                      # [c = 2, N = 1, E = 4]
    assert np.array_equal(accumulate(np.float32([[1, 1, 1, 1]]), g, 0.5, False), np.float32([[2.5, 1, 2, 3]]))
    assert np.array_equal(accumulate(np.zeros((1, 4), np.float32), g, 2.0, True), np.float32([[10, 16, 20, 32]]))
    acc = np.float32([1, -1, 2, 0, 3, 1, -2, 2]).reshape(1, 1, 2, 4)        # [T, N, C = 2, HW = 4]
    x, b = np.float32([2, 2, 2, 2, 1, 1, 1, 1]).reshape(1, 2, 4), np.float32([1, 0, 1, 0, 0, 0, 0, 3]).reshape(1, 2, 4)
    attr, maps, sums = finish(acc, x, b, 0)
    assert np.array_equal(attr.reshape(-1), np.float32([1, -2, 2, 0, 3, 1, -2, -4]))
    assert np.array_equal(maps.reshape(-1), np.float32([4, 3, 4, 4])) and sums.dtype == np.float64 and sums[0, 0] == -1.0
    attr, maps, sums = finish(acc, None, None, 1)
    assert np.array_equal(attr, acc) and sums[0, 0] == 6.0


def test_the_restatements_quadrature_gap_shrinks_from_4_to_64_steps():
    """The case tests/test_attr_gpu.py runs on the engine, chosen here so that the float64 restatement itself converges:
    max |delta| 4.625e-01 at 4 steps, 4.409e-02 at 64, ratio 10.5 (required: at least 2)."""
    model, derm, clinic, tc = convergence_case()
    fn = baseline_fn(model, torch.float64)
    zero = torch.zeros(1, 3, CONV_SIZE, CONV_SIZE, dtype=torch.float64)
    gap = {s: float(ref_integrated_gradients(fn, derm.double(), clinic.double(), zero, zero, tc, s)["delta"].abs().max())
           for s in (4, 64)}
    print(f"restatement max |delta|: {gap[4]:.3e} at 4 steps, {gap[64]:.3e} at 64, ratio {gap[4] / gap[64]:.1f}")
    assert gap[4] >= 2 * gap[64], gap


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
    for name in ENTRY_POINTS + ("sm3_attr_finish_blocks",):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text)
        assert name in L.SIGNATURES
        assert hasattr(lib, name)
    assert lib.sm3_abi_version() == 9  # additive: the version stays
    from sm3hip import attr, ops
    assert callable(attr.integrated_gradients) and callable(attr.smooth_grad)
    assert all(callable(getattr(ops, n)) for n in ("attr_path", "attr_noise", "attr_accumulate", "attr_finish"))


def _p(v):
    return C.c_void_p(v) if v else C.c_void_p(0)


def _path(lib, x=0x1000, base=0x2000, base_n=1, out=0x3000, N=2, E=64, k0=0, c=4, steps=8):
    return lib.sm3_attr_path(_p(x), _p(base), base_n, _p(out), N, E, k0, c, steps, C.c_void_p(0))


def _noise(lib, x=0x1000, sigma=0x2000, out=0x3000, N=2, E=64, k0=0, c=4, stride=1, seed=5):
    return lib.sm3_attr_noise(_p(x), _p(sigma), _p(out), N, E, k0, c, stride, seed, C.c_void_p(0))


def _accumulate(lib, g=0x1000, acc=0x2000, c=4, N=2, E=64, w=0.5, squared=0):
    return lib.sm3_attr_accumulate(_p(g), _p(acc), c, N, E, w, squared, C.c_void_p(0))


def _finish(lib, acc=0x1000, x=0x2000, base=0x3000, base_n=1, attr=0x4000, maps=0x5000, sums=0x6000, partials=0x7000, T=8,
            N=2, Cn=3, HW=64, mode=0):
    return lib.sm3_attr_finish(_p(acc), _p(x), _p(base), base_n, _p(attr), _p(maps), _p(sums), _p(partials), T, N, Cn, HW, mode,
                               C.c_void_p(0))


@pytest.mark.parametrize("kw,code", [
    (dict(x=0), -1), (dict(base=0), -1), (dict(out=0), -1), (dict(N=0), -1), (dict(E=0), -1), (dict(c=0), -1), (dict(steps=0), -1),
    (dict(k0=-1), -1), (dict(k0=5, c=4, steps=8), -1), (dict(base_n=3), -1), (dict(steps=2 ** 24, c=1), -1),
    (dict(N=2 ** 20, E=2 ** 20), -1), (dict(c=2 ** 20, steps=2 ** 20, N=2 ** 12, E=2 ** 22), -1),
    (dict(E=62), -2), (dict(x=0x1004), -2), (dict(out=0x3008), -2), (dict(base=0x2004), -2)])
def test_path_rejects_bad_arguments_before_any_launch(kw, code):
    assert _path(_lib(), **kw) == code, kw


@pytest.mark.parametrize("kw,code", [
    (dict(x=0), -1), (dict(sigma=0), -1), (dict(out=0), -1), (dict(N=-1), -1), (dict(E=0), -1), (dict(c=0), -1), (dict(k0=-2), -1),
    (dict(stride=0), -1), (dict(k0=2 ** 31 - 2, c=3), -1), (dict(N=2 ** 20, E=2 ** 20), -1), (dict(E=66), -2),
    (dict(x=0x1008), -2), (dict(out=0x3004), -2)])
def test_noise_rejects_bad_arguments_before_any_launch(kw, code):
    assert _noise(_lib(), **kw) == code, kw


@pytest.mark.parametrize("kw,code", [
    (dict(g=0), -1), (dict(acc=0), -1), (dict(c=0), -1), (dict(N=0), -1), (dict(E=-4), -1), (dict(squared=2), -1),
    (dict(N=2 ** 20, E=2 ** 20), -1), (dict(E=6), -2), (dict(g=0x1004), -2), (dict(acc=0x2008), -2)])
def test_accumulate_rejects_bad_arguments_before_any_launch(kw, code):
    assert _accumulate(_lib(), **kw) == code, kw


@pytest.mark.parametrize("kw,code", [
    (dict(acc=0), -1), (dict(attr=0), -1), (dict(maps=0), -1), (dict(sums=0), -1), (dict(partials=0), -1), (dict(x=0), -1),
    (dict(base=0), -1), (dict(T=0), -1), (dict(N=0), -1), (dict(Cn=0), -1), (dict(HW=0), -1), (dict(mode=2), -1),
    (dict(base_n=5), -1), (dict(T=2 ** 10, N=2 ** 10), -1), (dict(Cn=2 ** 20, HW=2 ** 24), -1),
    (dict(HW=66), -2), (dict(acc=0x1004), -2), (dict(x=0x2008), -2), (dict(sums=0x6004), -2)])
def test_finish_rejects_bad_arguments_before_any_launch(kw, code):
    assert _finish(_lib(), **kw) == code, kw


def test_finish_takes_no_images_in_smoothgrad_mode_and_sizes_its_workspace():
    lib = _lib()
    assert _finish(lib, x=0, base=0, mode=1, HW=62) == -2  # past the null checks: refused for the size, nothing launched
    assert [lib.sm3_attr_finish_blocks(hw) for hw in (4, 1024, 1028, 224 * 224)] == [1, 1, 2, 49]
    assert lib.sm3_attr_finish_blocks(0) == -1


# ---- the driver's host logic ------------------------------------------------------------------------------------------------
def test_chunk_planner():
    from sm3hip.attr import _pair_bytes, plan_chunk
    assert plan_chunk(32, 8, 100, 10 ** 9) == 32                 # everything fits: one chunk
    assert plan_chunk(32, 8, 10 ** 6, 64 * 10 ** 6) == 4         # half of the free memory / (8 pairs x 1 MB)
    assert plan_chunk(32, 8, 10 ** 6, 10 ** 3) == 1              # never below one path point
    assert plan_chunk(32, 8, 10 ** 6, 0) == 1 and plan_chunk(1, 1, 1, 10 ** 12) == 1
    assert plan_chunk(32, 8, 10 ** 6, 64 * 10 ** 6, share=1.0) == 8
    assert [plan_chunk(16, n, 10 ** 6, 32 * 10 ** 6) for n in (1, 2, 4, 16, 64)] == [16, 8, 4, 1, 1]
    assert _pair_bytes(1000, 12) == 3 * 1000 + 144
    for bad in (dict(steps=0), dict(n=0), dict(image_bytes=0)):
        with pytest.raises(ValueError):
            plan_chunk(**{**dict(steps=4, n=1, image_bytes=1, free_bytes=1), **bad})


def test_forward_measured_leaves_the_cycle_collector_as_it_found_it(monkeypatch):
    """The records' size is a difference of the allocator's counter taken with the collector off; it comes back on (or stays
    off) as the caller had it, also when the forward raises."""
    import gc
    from sm3hip.explain import forward_measured
    readings = iter([1000, 1000 + 2 * 4096, 0, 0, 0])
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda dev=None: next(readings))

    class Eng:
        def __init__(self, fail=False):
            self.fail = fail

        def encoder_only(self, lane, x, train, keep):
            assert not gc.isenabled()
            if self.fail:
                raise RuntimeError("forward failed")
            return x * 2, object()

    x = torch.ones(2, 3)
    was_on = gc.isenabled()
    try:
        gc.enable()
        f, per_image = forward_measured(Eng(), x)
        assert gc.isenabled() and per_image == 4096 and torch.equal(f, x * 2)
        with pytest.raises(RuntimeError):
            forward_measured(Eng(fail=True), x)
        assert gc.isenabled()
        gc.disable()
        forward_measured(Eng(), x)
        assert not gc.isenabled()
    finally:
        gc.enable() if was_on else gc.disable()


def test_drivers_refuse_train_mode_cpu_tensors_and_bad_arguments():
    from sm3hip.attr import integrated_gradients, smooth_grad
    from src.models.baseline import Baseline
    m = Baseline("resnet18", None)
    x = torch.zeros(2, 3, 32, 32)
    for fn, who in ((integrated_gradients, "integrated_gradients"), (smooth_grad, "smooth_grad")):
        with pytest.raises(ValueError, match=who + ".*eval mode"):
            fn(m.train(), x, x)
        m.eval()
        with pytest.raises(ValueError, match=who + ".*CUDA tensor"):
            fn(m, x, x)
        with pytest.raises(TypeError, match="Baseline"):
            fn(torch.nn.Linear(2, 2), x, x)
    with pytest.raises(ValueError, match="steps"):
        integrated_gradients(m, x, x, steps=0)
    with pytest.raises(ValueError, match="baseline"):
        integrated_gradients(m, x, x, baseline="black")
    with pytest.raises(ValueError, match="samples"):
        smooth_grad(m, x, x, samples=0)
    with pytest.raises(ValueError, match="sigma"):
        smooth_grad(m, x, x, sigma=-0.1)
    with pytest.raises(ValueError, match="seed"):
        smooth_grad(m, x, x, seed=-1)


# ---- the tools ----------------------------------------------------------------------------------------------------------
def _tool(name):
    spec = importlib.util.spec_from_file_location(f"sm3_{name}_cpu", os.path.join(TOOLS, f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_backbone_attr_parser_takes_backbone_cam_line_with_the_attribution_flags():
    ba = _tool("backbone_attr")
    a = ba.get_parser().parse_args(["--data-path", "-", "--data-name", "synthetic"])
    assert (a.method, a.steps, a.samples, a.sigma, a.squared, a.attr_seed, a.chunk, a.target, a.split, a.max_cases,
            a.linear_path, a.arch) == ("ig", 32, 16, 0.15, False, 0, None, "pred", "test", 64, None, "resnet50")
    assert not hasattr(a, "cam_layer")
    a = ba.get_parser().parse_args(["--data-path", "x", "--data-name", "SevenPCBaseDataset", "--method", "smoothgrad",
                                    "--samples", "8", "--sigma", "0.2", "--squared", "--attr-seed", "9", "--chunk", "2",
                                    "--target", "cls", "--split", "valid", "--max-cases", "5", "--linear-path", "p.pth",
                                    "-a", "resnet18", "--img-sz", "64", "96", "--amp", "--amp-dtype", "bf16"])
    assert (a.method, a.samples, a.sigma, a.squared, a.attr_seed, a.chunk, a.target, a.split, a.max_cases, a.linear_path,
            a.arch, a.img_sz) == ("smoothgrad", 8, 0.2, True, 9, 2, "cls", "valid", 5, "p.pth", "resnet18", [64, 96])


def test_mlc_attr_parser_takes_mlc_cam_line_with_the_attribution_flags():
    ma = _tool("mlc_attr")
    a = ma.get_parser().parse_args(["--data-path", "-", "--data-name", "synthetic"])
    assert (a.checkpoint, a.method, a.steps, a.mlc_proj, a.arch, a.test_sz, a.log_path) == (
        None, "ig", 32, "v4", "resnet50", 224, "./logs/mlc_attr")
    a = ma.get_parser().parse_args(["--data-path", "-", "--data-name", "synthetic", "--checkpoint", "c.pth", "--mlc-proj", "v2",
                                    "--mlc-proj-dim", "512", "--sa-dim-ff", "128", "--method", "ig", "--steps", "16",
                                    "--test-sz", "96", "--target", "cls", "--l2-norm", "--chunk", "4"])
    assert (a.checkpoint, a.mlc_proj, a.mlc_proj_dim, a.steps, a.test_sz, a.target, a.l2_norm, a.chunk) == (
        "c.pth", "v2", 512, 16, 96, "cls", True, 4)


@pytest.fixture
def no_gpu(monkeypatch):
    """Anything that reaches for the device fails the test."""
    def boom(*a, **k):
        raise AssertionError("touched the GPU before refusing")
    monkeypatch.setattr(torch, "Generator", boom)
    monkeypatch.setattr(torch.cuda, "synchronize", boom)
    monkeypatch.setattr(torch.nn.Module, "to", boom)
    from sm3hip import attr
    monkeypatch.setattr(attr, "integrated_gradients", boom)
    monkeypatch.setattr(attr, "smooth_grad", boom)


ATTR_REFUSALS = [
    (["--method", "occlusion"], "method"),
    (["--max-cases", "0"], "max-cases"),
    (["--steps", "0"], "steps"),
    (["--method", "smoothgrad", "--samples", "0"], "samples"),
    (["--steps", "8", "--chunk", "9"], "chunk"),
    (["--chunk", "0"], "chunk"),
    (["--method", "smoothgrad", "--sigma", "-1"], "sigma"),
    (["--attr-seed", "-1"], "attr-seed"),
]


@pytest.mark.parametrize("argv,msg", ATTR_REFUSALS + [
    (["--linear-path", "/nonexistent/best_linear.pth"], "does not exist"),
    (["-a", "resnext50_32x4d"], "not supported"),
])
def test_backbone_attr_refusals_stop_before_any_kernel(argv, msg, no_gpu, tmp_path):
    ba = _tool("backbone_attr")
    with pytest.raises(SystemExit, match=msg):
        ba.main(["--data-name", "synthetic", "--data-path", "-"] + argv + ["--log-path", str(tmp_path)])


@pytest.mark.parametrize("argv,msg", ATTR_REFUSALS + [
    (["--checkpoint", "/nonexistent/best_finetune.pth"], "does not exist"),
    (["-a", "resnet18"], "not supported"),
    (["--mlc-proj", "v9"], "mlc-proj"),
    (["--mlc-proj", "v0", "--mlc-proj-dim", "512"], "v0"),
])
def test_mlc_attr_refusals_stop_before_any_kernel(argv, msg, no_gpu, tmp_path):
    ma = _tool("mlc_attr")
    with pytest.raises(SystemExit, match=msg):
        ma.main(["--data-name", "synthetic", "--data-path", "-"] + argv + ["--log-path", str(tmp_path)])


@pytest.mark.parametrize("tool,flag", [("backbone_attr", "linear-path"), ("mlc_attr", "checkpoint")])
def test_real_data_needs_weights(tool, flag, no_gpu, tmp_path):
    root = tmp_path / "7PC"
    os.makedirs(root / "images")
    for f in ("meta.csv", "train_indexes.csv", "valid_indexes.csv", "test_indexes.csv"):
        (root / f).write_text("")
    with pytest.raises(SystemExit, match=flag):
        _tool(tool).main(["--data-name", "SevenPCBaseDataset", "--data-path", str(root), "--log-path", str(tmp_path)])


@pytest.mark.parametrize("tool", ["backbone_attr", "mlc_attr"])
def test_unknown_data_is_refused_and_cam_layer_is_not_a_flag(tool, no_gpu, tmp_path, capsys):
    mod = _tool(tool)
    with pytest.raises(SystemExit, match="not available"):
        mod.main(["--data-name", "ImageNet", "--data-path", "-", "--log-path", str(tmp_path)])
    with pytest.raises(SystemExit) as e:
        mod.main(["--data-name", "synthetic", "--data-path", "-", "--cam-layer", "layer4"])
    assert e.value.code == 2 and "--cam-layer" in capsys.readouterr().err
