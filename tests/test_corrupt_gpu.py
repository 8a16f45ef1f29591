"""GPU: the image corruptions of the robustness report (csrc/corrupt.hip, sm3hip/corrupt.py, the --corrupt flags of backbone_eval
and mlc_eval).

  * every corruption with new device code == its numpy restatement (tests/corrupt_inputs.py) bit for bit -- gaussian_noise within
    sigma * 1e-6 -- and the four colour corruptions == augment's _colour_finish on the equivalent AugParams, at the smallest shapes
    at which each kernel can go wrong: every read clamped, smaller than a JPEG block and than the largest kernel, exactly one
    block, one past a block edge, past an LDS tile edge with an element tail, several tiles;
  * the paths those shapes do not reach: more cases than one taps launch takes, every tile side of the pixelate kernel;
  * a case alone, first or last in a batch gives equal bits; ids, seed and modality change the noises; the modality changes
    neither the motion direction nor the cast sign;
  * store_corrupted on the hand-built arena of tests/tta_inputs.py; predict_split on the ResNet-18 Baseline and the ResNet-50
    inference.py Model; robustness_report against a plain-Python recount; one run of each tool on a derm7pt-shaped tree."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
DEV = "cuda:0"
MEAN, STD = [0.7833, 0.6712, 0.6026], [0.2139, 0.2472, 0.2571]
NEW_KERNELS = ["impulse_noise", "colour_cast", "defocus_blur", "motion_blur", "pixelate", "jpeg"]
COLOURS = {"darken": 1, "brighten": 1, "contrast": 2, "desaturate": 3}
SEED = 0x1234567887654321


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CI = _load("sm3_corrupt_inputs_gpu", os.path.join(ROOT, "tests", "corrupt_inputs.py"))
TI = _load("sm3_corrupt_tta_inputs", os.path.join(ROOT, "tests", "tta_inputs.py"))


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view(np.uint32)


def _apply(x, name, s, ids=None, seed=0, modality=0):
    from sm3hip import corrupt
    out = corrupt.apply(torch.from_numpy(x).to(DEV), name, s, ids, seed, modality)
    torch.cuda.synchronize()
    assert out.shape == x.shape and out.dtype == torch.float32
    return out.cpu().numpy()


def _ids(B):
    return [7, 2 ** 32 - 1, 3, 100000][:B]


def _severities(shape):
    return (1, 2, 3, 4, 5) if shape == CI.ALL_SEVERITIES_AT else (1, 5)


# ---- 1. equality with the restatements ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NEW_KERNELS)
@pytest.mark.parametrize("shape", CI.SHAPES)
def test_kernels_equal_the_numpy_restatement_bit_for_bit(shape, name):
    B, H, W = shape
    x = CI.images(B, H, W)
    assert (x == 0).any() or x.size == 3 and (x == 1).any()
    for s in _severities(shape):
        for modality in (0, 1):
            got = _apply(x, name, s, _ids(B), SEED, modality)
            want = CI.corrupt(x, name, s, _ids(B), SEED, modality)
            assert np.array_equal(_bits(got), _bits(want)), (name, s, modality, int((_bits(got) != _bits(want)).sum()))
            assert got.min() >= 0 and got.max() <= 1


@pytest.mark.parametrize("shape", CI.SHAPES)
def test_gaussian_noise_within_the_normals_bound(shape):
    """x + sigma z with z held to 1e-6 absolute (the bound tests/test_attr_gpu.py holds the same normals to): sigma * 1e-6 on the
    sum; the clamp moves no two values further apart, so the bound is asserted on what the kernel returns."""
    B, H, W = shape
    x = CI.images(B, H, W)
    for s in _severities(shape):
        sigma = CI.TABLE["gaussian_noise"][s - 1]
        for modality in (0, 1):
            got = _apply(x, "gaussian_noise", s, _ids(B), SEED, modality)
            raw, want = CI.gaussian_noise(x, s, _ids(B), SEED, modality)
            err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
            print(f"gaussian_noise {shape} s={s} m={modality}: max |device - numpy| {err:.3e} (bound {sigma * 1e-6:.1e}), "
                  f"{int((_bits(got) != _bits(want)).sum())} of {got.size} elements differ in a bit, clamped {float((raw != want).mean()):.3f}")
            assert err <= sigma * 1e-6, (s, modality, err)
            assert got.min() >= 0 and got.max() <= 1


def test_motion_blur_reaches_all_eight_directions():
    first = {}
    for i, k in enumerate(CI.direction(np.arange(400), 3, SEED)):
        first.setdefault(int(k), i)
    ids = [first[k] for k in range(8)]
    x = CI.images(8, 9, 17, seed=2)
    from sm3hip import corrupt
    for s in (1, 3, 5):
        if s == 3:
            assert [int(k) for k in CI.direction(ids, s, SEED)] == list(range(8))
            assert [int(w) & 7 for w in corrupt.case_words(np.array(ids), "motion_blur", s, SEED)] == list(range(8))
        got, want = _apply(x, "motion_blur", s, ids, SEED), CI.motion_blur(x, s, ids, SEED)
        assert np.array_equal(_bits(got), _bits(want)), s
    # every direction by its own table, whatever the case word: the entry point with the table index given
    from sm3hip import ops
    tables, counts = corrupt.tap_tables("motion_blur", 5)
    out = torch.empty(8, 3, 9, 17, device=DEV)
    ops.corrupt_taps(torch.from_numpy(x).to(DEV), tables, counts, np.arange(8, dtype=np.int32), out)
    torch.cuda.synchronize()
    for k in range(8):
        assert np.array_equal(_bits(out[k]), _bits(CI.taps_mean(x[k], CI.line(21, k)))), k


@pytest.mark.parametrize("name", list(COLOURS))
def test_colour_corruptions_equal_the_existing_colour_finish(name):
    """Normalize with mean 0 and std 1 is (v - 0) / 1 = v to the bit, so _colour_finish returns the colour op's own output."""
    from sm3hip.augment import AugParams, SimCLRAugment
    for B, H, W in CI.SHAPES:
        x = torch.from_numpy(CI.images(B, H, W)).to(DEV)
        for s in _severities((B, H, W)):
            p = AugParams()
            p.ops, p.factors = torch.zeros(4, B, dtype=torch.int32), torch.ones(4, B)
            p.ops[0], p.factors[0] = COLOURS[name], CI.TABLE[name][s - 1]
            p.gray, p.sigma = torch.zeros(B, dtype=torch.uint8), torch.zeros(B)
            want = SimCLRAugment((H, W), [0.0] * 3, [1.0] * 3)._colour_finish(x.clone(), p, p.ops.to(DEV), p.factors.to(DEV),
                                                                             p.gray.to(DEV), p.sigma.to(DEV))
            got = _apply(x.cpu().numpy(), name, s, _ids(B), SEED)
            assert np.array_equal(_bits(got), _bits(want)), (name, (B, H, W), s)


# ---- 2. index independence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CI.NAMES)
def test_a_case_does_not_depend_on_its_batch_or_position(name):
    H, W = 33, 31
    x = CI.images(3, H, W, seed=4)
    ids = [11, 500, 2 ** 31 + 5]
    for s in (1, 5):
        whole = _apply(x, name, s, ids, SEED, 1)
        for b in range(3):
            alone = _apply(x[b:b + 1], name, s, ids[b:b + 1], SEED, 1)
            assert np.array_equal(_bits(alone[0]), _bits(whole[b])), (name, s, b)
        back = _apply(x[::-1].copy(), name, s, ids[::-1], SEED, 1)  # first becomes last
        assert np.array_equal(_bits(back[::-1]), _bits(whole)), (name, s)
        tail = _apply(x[1:].copy(), name, s, ids[1:], SEED, 1)      # another chunk
        assert np.array_equal(_bits(tail), _bits(whole[1:])), (name, s)


def test_ids_seed_and_modality_change_the_noises_only():
    x = CI.images(2, 16, 24, seed=5)
    for name in ("gaussian_noise", "impulse_noise"):
        base = _apply(x, name, 3, [4, 9], 77, 0)
        assert np.array_equal(_bits(base), _bits(_apply(x, name, 3, [4, 9], 77, 0)))
        for other in (_apply(x, name, 3, [5, 9], 77, 0)[0], _apply(x, name, 3, [4, 9], 78, 0)[0], _apply(x, name, 3, [4, 9], 77, 1)[0],
                      _apply(x, name, 3, [4, 9], 77 + (1 << 32), 0)[0]):
            assert not np.array_equal(_bits(other), _bits(base[0])), name
        assert np.array_equal(_bits(_apply(x, name, 3, [5, 9], 77, 0)[1]), _bits(base[1]))  # the other case is untouched
        assert np.array_equal(_bits(_apply(x, name, 3, None, 77, 0)), _bits(_apply(x, name, 3, [0, 1], 77, 0)))  # the default ids
    ids = list(range(16))
    x = CI.images(16, 5, 7, seed=6)
    for name in ("motion_blur", "colour_cast"):  # the case word is shared by the modalities of a case
        assert np.array_equal(_bits(_apply(x, name, 4, ids, 77, 0)), _bits(_apply(x, name, 4, ids, 77, 1))), name
        assert not np.array_equal(_bits(_apply(x, name, 4, ids, 77, 0)), _bits(_apply(x, name, 4, ids, 78, 0))), name
    for name in ("defocus_blur", "pixelate", "jpeg", "darken"):  # nothing random in these
        assert np.array_equal(_bits(_apply(x, name, 2, ids, 1, 0)), _bits(_apply(x, name, 2, ids[::-1], 2, 1))), name


def test_taps_past_the_64_case_launch_and_pixelate_at_every_tile_side():
    """The paths the table's shapes do not reach: sm3_corrupt_taps sends 64 cases per launch (their table numbers travel in the
    kernel arguments), so case 64 and 65 are in a second launch; sm3_corrupt_pixelate's tile is (32 / f) * f pixels a side -- 30
    for f = 3, 5 and 6, 32 for f = 1, 2, 4, 8, 16, 32 -- and 70 x 70 needs several of each."""
    from sm3hip import ops
    x = CI.images(66, 5, 7, seed=8)
    ids = list(range(100, 166))
    assert len(set(int(k) for k in CI.direction(ids, 2, SEED))) == 8
    for name in ("motion_blur", "defocus_blur"):
        whole = _apply(x, name, 2, ids, SEED)
        assert np.array_equal(_bits(whole), _bits(CI.corrupt(x, name, 2, ids, SEED))), name
        assert np.array_equal(_bits(_apply(x[65:], name, 2, ids[65:], SEED)[0]), _bits(whole[65])), name
    for B, H, W in ((1, 70, 70), (1, 33, 31)):
        x = CI.images(B, H, W, seed=9)
        for f in (1, 3, 5, 6, 16, 32):
            out = torch.empty(B, 3, H, W, device=DEV)
            ops.corrupt_pixelate(torch.from_numpy(x).to(DEV), f, out)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(out), _bits(CI.pixelate_f(x, f))), (H, W, f)
        assert np.array_equal(_bits(CI.pixelate_f(x, 1)), _bits(x))


def test_entry_points_launch_nothing_when_they_refuse():
    from sm3hip import _lib, corrupt, ops
    x = torch.from_numpy(CI.images(2, 5, 7)).to(DEV)
    out = torch.full_like(x, 7.0)
    lib, st = _lib.load(), ops._stream()
    ids = torch.zeros(2, dtype=torch.int32, device=DEV)
    tables, counts = corrupt.tap_tables("defocus_blur", 1)
    bad_index = np.array([0, 1], np.int32)
    ql, qc = corrupt.quant_tables(25)
    rcs = [lib.sm3_corrupt_pointwise(ops._ptr(x), 2, 5, 7, ops._ptr(ids), 0, 6, 0.08, 1, 0, ops._ptr(out), st),
           lib.sm3_corrupt_taps(ops._ptr(x), 2, 5, 7, tables.ctypes.data, counts.ctypes.data, 1, tables.shape[1], bad_index.ctypes.data,
                                ops._ptr(out), st),
           lib.sm3_corrupt_pixelate(ops._ptr(x), 2, 5, 7, 0, ops._ptr(out), st),
           lib.sm3_corrupt_jpeg(ops._ptr(x), 2, 5, 7, 0, ql.ctypes.data, qc.ctypes.data, ops._ptr(out), st)]
    torch.cuda.synchronize()
    assert rcs == [-1] * 4 and bool((out == 7.0).all())
    with pytest.raises(ValueError, match="another tensor"):
        ops.corrupt_pixelate(x, 2, x)


# ---- 3. the image store ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arena():
    a, offset, hs, ws = TI.arena()
    return a.to(DEV), offset, hs, ws


INDEX = [0, 1, 2, 3, 4, 2]


@pytest.mark.parametrize("size", [(17, 17), (9, 17)])
def test_store_corrupted_on_a_hand_built_arena(arena, size):
    from sm3hip import corrupt
    from sm3hip.augment import SimCLRAugment, whole_image_params
    a, offset, hs, ws = arena
    idx = torch.tensor(INDEX)
    aug = SimCLRAugment(size, MEAN, STD)
    params = whole_image_params(hs[idx], ws[idx])
    want = aug.apply_ragged(a, offset, hs, ws, idx.int(), params)
    got = corrupt.store_corrupted(a, offset, hs, ws, INDEX, size, MEAN, STD, None, None, None)
    assert got.shape == (len(INDEX), 3) + size and np.array_equal(_bits(got), _bits(want))  # the validation batch, bit for bit
    ids = [3, 1, 4, 1, 5, 9]
    img, on_device = aug.resample_ragged(a, offset, hs, ws, idx.int(), params)
    assert float(img.min()) >= 0 and float(img.max()) <= 1
    for name, s in (("jpeg", 5), ("gaussian_noise", 2), ("motion_blur", 3), ("pixelate", 1)):
        got = corrupt.store_corrupted(a, offset, hs, ws, INDEX, size, MEAN, STD, name, s, ids, seed=3, modality=1)
        want = aug._colour_finish(corrupt.apply(img, name, s, ids, 3, 1), params, *on_device)
        assert np.array_equal(_bits(got), _bits(want)), name
        if name != "gaussian_noise":  # the restatement on the resampled image, then Normalize as (v - mean) / std
            r = CI.corrupt(img.cpu().numpy(), name, s, ids, 3, 1)
            norm = ((r - np.float32(MEAN)[None, :, None, None]) / np.float32(STD)[None, :, None, None]).astype(np.float32)
            assert np.array_equal(_bits(got), _bits(norm)), name
    for name, s in (("darken", 4), ("contrast", 2), ("desaturate", 5)):  # AugParams with one ops / factors entry
        p = whole_image_params(hs[idx], ws[idx])
        p.ops[0], p.factors[0] = COLOURS[name], CI.TABLE[name][s - 1]
        want = aug.apply_ragged(a, offset, hs, ws, idx.int(), p)
        got = corrupt.store_corrupted(a, offset, hs, ws, INDEX, size, MEAN, STD, name, s, ids)
        assert np.array_equal(_bits(got), _bits(want)), name


# ---- 4. predict_split -----------------------------------------------------------------------------------------------------------
TTA = _load("sm3_corrupt_tta_gpu_helpers", os.path.join(ROOT, "tests", "test_tta_gpu.py"))
N_CASES = 12


def _split(arena):
    from types import SimpleNamespace
    from sm3hip.imagestore import StoreSplit
    a, offset, hs, ws = arena
    store = SimpleNamespace(arena=a, offset=offset, img_h=hs, img_w=ws)
    derm_ids = torch.tensor([(3 * i) % 5 for i in range(N_CASES)], dtype=torch.int32)
    clinic_ids = torch.tensor([(2 * i + 1) % 5 for i in range(N_CASES)], dtype=torch.int32)
    labels = torch.stack([(torch.arange(N_CASES) * 7 // 3) % n for n in TI.NUM_CLASSES], dim=1).to(DEV)
    return store, StoreSplit(derm_ids, clinic_ids, labels)


def _same(a, b):
    return all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(a, b))


@pytest.fixture(scope="module")
def record18(arena):
    """predict_split of the ResNet-18 Baseline under every corruption at severities 1 and 5, shared by the tests below."""
    from sm3hip import corrupt
    model, forward, _ = TTA._baseline18()
    store, split = _split(arena)
    rec = corrupt.predict_split(model, store, split, (32, 32), MEAN, STD, "all", (1, 5), "both", seed=9, batch_size=5)
    return model, forward, store, split, rec


def test_predict_split_on_the_resnet18_baseline(arena, record18):
    from sm3hip import corrupt, tta
    model, forward, store, split, rec = record18
    a, offset, hs, ws = arena
    assert sorted(rec) == ["clean", "modality", "preds", "seed", "targets"] and rec["modality"] == "both" and rec["seed"] == 9
    assert list(rec["preds"]) == [(n, s) for n in CI.NAMES for s in (1, 5)] and torch.equal(rec["targets"], split.labels)
    none = tta.predict_split(model, store, split, (32, 32), MEAN, STD, "none", 1, 0.8, batch_size=7)
    for t in range(8):
        assert rec["clean"][t].shape == (N_CASES, TI.NUM_CLASSES[t])
        assert np.array_equal(_bits(rec["clean"][t]), _bits(none["logits"][t][:, 0])), t
    pos = list(range(N_CASES))
    with torch.no_grad():
        for key in (("jpeg", 5), ("gaussian_noise", 1), ("motion_blur", 5), ("darken", 1), ("colour_cast", 5)):
            dv, cv = (corrupt.store_corrupted(a, offset, hs, ws, ids, (32, 32), MEAN, STD, key[0], key[1], pos, 9, m)
                      for m, ids in enumerate((split.derm_ids, split.clinic_ids)))
            assert _same(rec["preds"][key], [o.float() for o in forward(dv, cv)]), key
            assert not _same(rec["preds"][key], rec["clean"]), key
    other = corrupt.predict_split(model, store, split, (32, 32), MEAN, STD, "all", (1, 5), "both", seed=9, batch_size=64)
    assert _same(other["clean"], rec["clean"]) and all(_same(other["preds"][k], rec["preds"][k]) for k in rec["preds"])


@pytest.mark.parametrize("modality", ["derm", "clinic"])
def test_predict_split_corrupts_one_modality_and_leaves_the_other_clean(arena, record18, modality, monkeypatch):
    from sm3hip import corrupt, tta
    model, forward, store, split, rec = record18
    a, offset, hs, ws = arena
    seen, view_logits = [], tta._view_logits
    monkeypatch.setattr(tta, "_view_logits", lambda sub, d, c, rows: seen.append((d.clone(), c.clone())) or view_logits(sub, d, c, rows))
    one = corrupt.predict_split(model, store, split, (32, 32), MEAN, STD, ["jpeg", "impulse_noise"], [5], modality, seed=9,
                                batch_size=N_CASES)
    assert _same(one["clean"], rec["clean"]) and one["modality"] == modality and len(seen) == 3
    hit = 0 if modality == "derm" else 1
    for d, c in seen[1:]:
        pair, clean = (d, c), seen[0]
        assert np.array_equal(_bits(pair[1 - hit]), _bits(clean[1 - hit]))      # the other image's bits are the clean ones
        assert not np.array_equal(_bits(pair[hit]), _bits(clean[hit]))
    pos = list(range(N_CASES))
    ids = (split.derm_ids, split.clinic_ids)
    with torch.no_grad():
        imgs = [corrupt.store_corrupted(a, offset, hs, ws, ids[m], (32, 32), MEAN, STD, "jpeg" if m == hit else None, 5, pos, 9, m)
                for m in (0, 1)]
        assert _same(one["preds"][("jpeg", 5)], [o.float() for o in forward(*imgs)])
    assert not _same(one["preds"][("jpeg", 5)], rec["preds"][("jpeg", 5)])


def test_predict_split_on_the_resnet50_model(arena):
    from sm3hip import corrupt, tta
    model, forward, _ = TTA._mlc50()
    store, split = _split(arena)
    a, offset, hs, ws = arena
    names = ["gaussian_noise", "defocus_blur", "jpeg", "desaturate"]
    rec = corrupt.predict_split(model, store, split, (32, 32), MEAN, STD, names, (1, 5), batch_size=5)
    none = tta.predict_split(model, store, split, (32, 32), MEAN, STD, "none", 1, 0.8, batch_size=N_CASES)
    assert _same(rec["clean"], [l[:, 0] for l in none["logits"]])
    pos = list(range(N_CASES))
    with torch.no_grad():
        for key in (("jpeg", 1), ("gaussian_noise", 5), ("desaturate", 5)):
            dv, cv = (corrupt.store_corrupted(a, offset, hs, ws, ids, (32, 32), MEAN, STD, key[0], key[1], pos, 0, m)
                      for m, ids in enumerate((split.derm_ids, split.clinic_ids)))
            assert _same(rec["preds"][key], [o.float() for o in forward(dv, cv)]), key
    other = corrupt.predict_split(model, store, split, (32, 32), MEAN, STD, names, (1, 5), batch_size=N_CASES)
    assert _same(other["clean"], rec["clean"]) and all(_same(other["preds"][k], rec["preds"][k]) for k in rec["preds"])
    with pytest.raises(ValueError, match="eval mode"):
        corrupt.predict_split(model.train(), store, split, (32, 32), MEAN, STD, ["jpeg"], [1])


# ---- 5. the report --------------------------------------------------------------------------------------------------------------
def test_robustness_report_against_a_plain_python_recount(record18):
    from sm3hip import corrupt, report
    rec = record18[4]
    keys = [("gaussian_noise", 1), ("gaussian_noise", 5), ("jpeg", 1), ("jpeg", 5), ("contrast", 5)]
    small = dict(rec, preds={k: rec["preds"][k] for k in keys})
    rep = corrupt.robustness_report(small, bootstrap=40, confidence=0.9, seed=3)
    N, targets = N_CASES, rec["targets"]
    clean = report.evaluation_report(rec["clean"], targets, 40, 0.9, 3)
    assert np.array_equal(rep["clean"]["values"].numpy(), clean["values"].numpy()) and rep["n"] == N
    assert rep["names"] == ["gaussian_noise", "jpeg", "contrast"] and rep["severities"] == [1, 5]
    iA, k8 = report.METRICS.index("AUC"), report.COLUMNS.index("8 avg")
    zc = torch.cat(rec["clean"], dim=1).cpu().numpy()
    for k in keys:
        cmp = report.compare(report.evaluation_report(rec["preds"][k], targets, 40, 0.9, 3), clean)
        for field in ("delta", "lo", "hi", "frac_le_zero"):
            assert np.array_equal(np.asarray(rep["compare"][k][field]), np.asarray(cmp[field]), equal_nan=True), (k, field)
        zk = torch.cat(rec["preds"][k], dim=1).cpu().numpy()
        q = TI.q_of(np.stack([zc, zk], axis=1))                      # [N, 2, 24], the fp64 restatement: within 1 of the device
        st, col, fr, dp = rep["stability"][k], 0, [], []
        for t, label in enumerate(corrupt.CLASSES_NAME):
            n_t = TI.NUM_CLASSES[t]
            flips = sum(1 for i in range(N) if int(zc[i, col:col + n_t].argmax()) != int(zk[i, col:col + n_t].argmax()))
            assert st["flips"][label] == flips and st["flip_rate"][label] == flips / N, (k, label)
            c = col + TI.CLS_WEIGHTS[t]
            total = sum(abs(int(q[i, 0, c]) - int(q[i, 1, c])) for i in range(N))
            assert abs(st["abs_dp_sum"][label] - total) <= 2 * N, (k, label)   # each of the 2 N integers within 1
            assert st["mean_abs_dp"][label] == st["abs_dp_sum"][label] / (N * TI.ONE)
            fr.append(st["flip_rate"][label]), dp.append(st["mean_abs_dp"][label])
            col += n_t
        for stat, vals in (("flip_rate", fr), ("mean_abs_dp", dp)):
            acc = 0.0
            for v in vals:
                acc = acc + v
            assert st[stat]["AVG"] == acc / 8
    d = lambda k: float(rep["compare"][k]["delta"][iA, k8])
    want = {"gaussian_noise": (d(keys[0]) + d(keys[1])) / 2, "jpeg": (d(keys[2]) + d(keys[3])) / 2, "contrast": d(keys[4]) / 1}
    assert rep["auc_drop"] == want
    assert rep["mean_drop"] == ((want["gaussian_noise"] + want["jpeg"]) + want["contrast"]) / 3
    rows = corrupt.csv_rows(rep)
    assert [(r["name"], r["severity"]) for r in rows] == keys and all("delta_lo" in r for r in rows)
    assert len(corrupt.stats_lines(rep)) == 3 and "mean_drop" in corrupt.stats_line(rep)
    plain = corrupt.robustness_report(small)
    assert "lo" not in plain["compare"][keys[0]] and plain["auc_drop"] == rep["auc_drop"]


# ---- 6. the tools ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    knn = _load("sm3_corrupt_knn_helpers", os.path.join(ROOT, "tests", "test_knn_gpu.py"))
    root = knn._write_tree(tmp_path_factory.mktemp("corrupt") / "7PC")
    return root, ["--data-name", "SevenPCBaseDataset", "--data-path", str(root), "-j", "4", "--mean"] + [str(m) for m in MEAN] + \
        ["--std"] + [str(s) for s in STD]


CORRUPT_FLAGS = ["--corrupt", "jpeg", "motion_blur", "--corrupt-severity", "1", "5"]
FILES = ["jpeg_1.pt", "jpeg_5.pt", "motion_blur_1.pt", "motion_blur_5.pt"]


def _check_outputs(log, labels, capsys_out):
    import json
    from sm3hip import report
    assert sorted(os.listdir(log / "val_predictions_corrupt")) == FILES
    plain = torch.load(log / "val_predictions.pt", weights_only=False)
    for f in FILES:
        saved = torch.load(log / "val_predictions_corrupt" / f, weights_only=False)
        assert sorted(saved) == ["AUC_AVG", "corrupt", "epoch", "preds", "targets"] and torch.equal(saved["targets"], labels)
        assert f == f"{saved['corrupt']['name']}_{saved['corrupt']['severity']}.pt" and saved["corrupt"]["modality"] == "both"
        preds, tg = report.load_predictions(str(log / "val_predictions_corrupt" / f))
        assert torch.equal(tg, labels) and all(torch.equal(p, q) for p, q in zip(preds, saved["preds"]))
        assert [tuple(p.shape) for p in preds] == [tuple(p.shape) for p in plain["preds"]]
        assert not all(torch.equal(p.float(), q.float()) for p, q in zip(preds, plain["preds"]))
    rob = json.load(open(log / "val_robustness.json"))
    assert rob["names"] == ["motion_blur", "jpeg"] and rob["severities"] == [1, 5] and rob["n"] == len(labels)
    assert len(rob["rows"]) == 4 and sorted(rob["auc_drop"]) == ["jpeg", "motion_blur"]
    lines = open(log / "val_robustness.csv").read().splitlines()
    assert lines[0].startswith("name,severity,AUC_AVG,delta_AUC_AVG") and len(lines) == 5
    assert capsys_out.count("val-corrupt motion_blur (both)") == 1 and capsys_out.count("val-corrupt jpeg (both)") == 1
    assert "mean_drop" in capsys_out


def test_backbone_eval_on_a_derm7pt_tree(tree, tmp_path, capsys):
    from src.utils.data.datasets import read_split
    root, data = tree
    labels = read_split(str(root), "test")[2]
    be = _load("sm3_corrupt_backbone_eval_tree", os.path.join(TOOLS, "backbone_eval.py"))
    run = lambda extra, out: be.main(data + ["-a", "resnet18", "-b", "6", "--img-sz", "32", "32", "--epochs", "1", "--finetune",
                                             "fc", "--seed", "3", "--bootstrap", "20", "--log-path", str(tmp_path / out)] + extra)
    run([], "plain")
    run(CORRUPT_FLAGS, "corrupt")
    out = capsys.readouterr().out
    _check_outputs(tmp_path / "corrupt", labels, out)
    plain = torch.load(tmp_path / "plain" / "val_predictions.pt", weights_only=False)
    same = torch.load(tmp_path / "corrupt" / "val_predictions.pt", weights_only=False)
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(plain["preds"], same["preds"]))  # the ordinary pass is untouched
    assert sorted(os.listdir(tmp_path / "corrupt")) == sorted(os.listdir(tmp_path / "plain") + ["val_predictions_corrupt",
                                                                                             "val_robustness.csv", "val_robustness.json"])
    er = _load("sm3_corrupt_eval_report", os.path.join(TOOLS, "eval_report.py"))
    er.main([str(tmp_path / "corrupt" / "val_predictions_corrupt" / "jpeg_5.pt"), "--against", str(tmp_path / "plain" / "val_predictions.pt"),
             "--significance", "--permutations", "200", "--out", str(tmp_path / "er")])
    assert "AUC difference" in capsys.readouterr().out
    with pytest.raises(SystemExit, match="real data set"):
        be.main(["--data-name", "synthetic", "--data-path", "-", "-a", "resnet18"] + CORRUPT_FLAGS)


def test_mlc_eval_on_a_derm7pt_tree(tree, tmp_path, capsys):
    from src.utils.data.datasets import read_split
    root, data = tree
    labels = read_split(str(root), "test")[2]
    me = _load("sm3_corrupt_mlc_eval_tree", os.path.join(TOOLS, "mlc_eval.py"))
    me.main(data + ["-b", "6", "--train-sz", "32", "--test-sz", "32", "--epochs", "1", "--mlc-proj-dim", "128", "--sa-dim-ff", "64",
                    "--log-path", str(tmp_path)] + CORRUPT_FLAGS)
    _check_outputs(tmp_path, labels, capsys.readouterr().out)
    er = _load("sm3_corrupt_eval_report_mlc", os.path.join(TOOLS, "eval_report.py"))
    er.main([str(tmp_path / "val_predictions_corrupt" / "motion_blur_5.pt"), "--against", str(tmp_path / "val_predictions.pt"),
             "--out", str(tmp_path / "er")])
    assert "AUC difference" in capsys.readouterr().out
