"""CPU: the image corruptions of the robustness report (sm3hip/corrupt.py, csrc/corrupt.hip) -- the tables as the module text
prints them, the tap lists, the quantisation tables against literal arrays, the DCT table in the kernel source against its
formula; the numpy restatement of the JPEG round trip (tests/corrupt_inputs.py) against Pillow's own; the blur and pixelate
restatements on constant and mirrored images; the four entry points declared, bound, exported and refusing bad arguments before
any launch; the host half of sm3hip.corrupt and the flags' refusals (each before anything touches the GPU)."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")
ENTRY_POINTS = ("sm3_corrupt_pointwise", "sm3_corrupt_taps", "sm3_corrupt_pixelate", "sm3_corrupt_jpeg")


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CI = _load("sm3_corrupt_inputs_cpu", os.path.join(ROOT, "tests", "corrupt_inputs.py"))


# ---- tables -------------------------------------------------------------------------------------------------------------------
def test_the_tables_are_as_printed():
    from sm3hip import corrupt
    assert list(corrupt.CORRUPTIONS) == CI.NAMES and [corrupt.CORRUPTIONS[n] for n in CI.NAMES] == list(range(11))
    assert corrupt.SEVERITIES == (1, 2, 3, 4, 5) and corrupt.STREAM == 7
    want = {"gaussian_noise": (0.08, 0.12, 0.18, 0.26, 0.38), "impulse_noise": (0.03, 0.06, 0.09, 0.17, 0.27),
            "defocus_blur": (3, 4, 6, 8, 10), "motion_blur": (5, 9, 13, 17, 21), "pixelate": (2, 3, 4, 6, 8),
            "jpeg": (25, 18, 15, 10, 7), "darken": (0.8, 0.65, 0.5, 0.35, 0.2), "brighten": (1.2, 1.4, 1.6, 1.8, 2.0),
            "contrast": (0.75, 0.6, 0.45, 0.3, 0.15), "desaturate": (0.8, 0.6, 0.4, 0.2, 0.0),
            "colour_cast": (0.05, 0.1, 0.15, 0.2, 0.3)}
    for name, row in want.items():
        assert tuple(corrupt.parameters(name, s) for s in corrupt.SEVERITIES) == row, name
    for bad in (("blur", 1), ("jpeg", 0), ("jpeg", 6), ("jpeg", True), ("jpeg", 1.0)):
        with pytest.raises(ValueError):
            corrupt.parameters(*bad)
    with pytest.raises(ValueError, match="not a blur"):
        corrupt.tap_tables("jpeg", 1)
    text = open(os.path.join(ROOT, "skin-sm3_amd", "sm3hip", "resample.py")).read()
    assert "7 the case and element words of sm3hip/corrupt.py" in text  # the stream is on the list


def test_tap_tables_are_the_disk_and_the_eight_lines():
    from sm3hip import corrupt
    for s, r in zip(corrupt.SEVERITIES, (3, 4, 6, 8, 10)):
        tables, counts = corrupt.tap_tables("defocus_blur", s)
        assert tables.dtype == np.int16 and counts.dtype == np.int32 and tables.shape == (1, int(counts[0]), 2)
        taps = [tuple(int(v) for v in t) for t in tables[0]]
        lattice = [(dy, dx) for dy in range(-10, 11) for dx in range(-10, 11) if dy * dy + dx * dx <= r * r]
        assert taps == lattice == CI.disk(r)  # exactly the lattice points, row-major
        assert np.abs(tables).max() <= 10
    assert int(corrupt.tap_tables("defocus_blur", 5)[1][0]) == 317
    for s, L in zip(corrupt.SEVERITIES, (5, 9, 13, 17, 21)):
        tables, counts = corrupt.tap_tables("motion_blur", s)
        assert tables.shape == (8, L, 2) and list(counts) == [L] * 8 and np.abs(tables).max() <= 10
        for k in range(8):
            assert [tuple(int(v) for v in t) for t in tables[k]] == CI.line(L, k)
            assert tuple(tables[k, L // 2]) == (0, 0) and np.array_equal(tables[k], -tables[k, ::-1])  # point-symmetric
        assert [tuple(t) for t in tables[0]] == [(0, t) for t in range(-(L // 2), L // 2 + 1)]           # k = 0: along x
        assert [tuple(t) for t in tables[4]] == [(t, 0) for t in range(-(L // 2), L // 2 + 1)]           # k = 4: along y
    assert [tuple(t) for t in corrupt.tap_tables("motion_blur", 1)[0][2]] == [(-1, -1), (-1, -1), (0, 0), (1, 1), (1, 1)]  # duplicates kept


QUANT = {
    25: ([32, 22, 20, 32, 48, 80, 102, 122, 24, 24, 28, 38, 52, 116, 120, 110, 28, 26, 32, 48, 80, 114, 138, 112, 28, 34, 44, 58, 102,
          174, 160, 124, 36, 44, 74, 112, 136, 218, 206, 154, 48, 70, 110, 128, 162, 208, 226, 184, 98, 128, 156, 174, 206, 242, 240,
          202, 144, 184, 190, 196, 224, 200, 206, 198],
         [34, 36, 48, 94, 198, 198, 198, 198, 36, 42, 52, 132, 198, 198, 198, 198, 48, 52, 112, 198, 198, 198, 198, 198, 94, 132, 198,
          198, 198, 198, 198, 198] + [198] * 32),
    18: ([44, 30, 28, 44, 66, 111, 141, 169, 33, 33, 39, 53, 72, 161, 166, 152, 39, 36, 44, 66, 111, 158, 191, 155, 39, 47, 61, 80, 141,
          241, 222, 172, 50, 61, 102, 155, 188, 255, 255, 213, 66, 97, 152, 177, 224, 255, 255, 255, 136, 177, 216, 241, 255, 255, 255,
          255, 199, 255, 255, 255, 255, 255, 255, 255],
         [47, 50, 66, 130, 255, 255, 255, 255, 50, 58, 72, 183, 255, 255, 255, 255, 66, 72, 155, 255, 255, 255, 255, 255, 130, 183, 255,
          255, 255, 255, 255, 255] + [255] * 32),
    15: ([53, 37, 33, 53, 80, 133, 170, 203, 40, 40, 47, 63, 87, 193, 200, 183, 47, 43, 53, 80, 133, 190, 230, 186, 47, 57, 73, 97, 170,
          255, 255, 206, 60, 73, 123, 186, 226, 255, 255, 255, 80, 117, 183, 213, 255, 255, 255, 255, 163, 213, 255, 255, 255, 255, 255,
          255, 240, 255, 255, 255, 255, 255, 255, 255],
         [57, 60, 80, 157, 255, 255, 255, 255, 60, 70, 87, 220, 255, 255, 255, 255, 80, 87, 186, 255, 255, 255, 255, 255, 157, 220, 255,
          255, 255, 255, 255, 255] + [255] * 32),
    10: ([80, 55, 50, 80, 120, 200, 255, 255, 60, 60, 70, 95, 130, 255, 255, 255, 70, 65, 80, 120, 200, 255, 255, 255, 70, 85, 110, 145,
          255, 255, 255, 255, 90, 110, 185, 255, 255, 255, 255, 255, 120, 175, 255, 255, 255, 255, 255, 255, 245, 255, 255, 255, 255, 255,
          255, 255] + [255] * 8,
         [85, 90, 120, 235, 255, 255, 255, 255, 90, 105, 130, 255, 255, 255, 255, 255, 120, 130, 255, 255, 255, 255, 255, 255, 235] +
         [255] * 39),
    7: ([114, 79, 71, 114, 171, 255, 255, 255, 86, 86, 100, 136, 186, 255, 255, 255, 100, 93, 114, 171, 255, 255, 255, 255, 100, 121,
         157, 207, 255, 255, 255, 255, 129, 157, 255, 255, 255, 255, 255, 255, 171, 250] + [255] * 22,
        [121, 129, 171, 255, 255, 255, 255, 255, 129, 150, 186, 255, 255, 255, 255, 255, 171, 186] + [255] * 46),
}


def test_quantisation_tables_at_the_five_qualities():
    from sm3hip import corrupt
    assert [corrupt.parameters("jpeg", s) for s in corrupt.SEVERITIES] == list(QUANT)
    for q, (luma, chroma) in QUANT.items():
        assert len(luma) == len(chroma) == 64
        got = corrupt.quant_tables(q)
        assert got[0].dtype == np.int32 and list(got[0]) == luma and list(got[1]) == chroma, q
        assert [list(t.reshape(-1)) for t in CI.quant(q)] == [luma, chroma]  # the restatement's own
    assert list(corrupt.quant_tables(50)[0]) == CI.K1 and list(corrupt.quant_tables(50)[1]) == CI.K2  # scale 100: Annex K itself
    assert set(corrupt.quant_tables(100)[0]) == {1} and int(corrupt.quant_tables(1)[0].min()) == 255
    for bad in (0, 101, 2.5, True):
        with pytest.raises(ValueError):
            corrupt.quant_tables(bad)


def test_the_kernels_dct_table_is_its_formula():
    text = open(os.path.join(ROOT, "skin-sm3_amd", "csrc", "corrupt.hip")).read()
    body = re.search(r"kC13\[64\]\s*=\s*\{(.*?)\};", text, flags=re.S).group(1)
    got = [int(v) for v in re.findall(r"-?\d+", re.sub(r"//.*", "", body))]
    assert got == [int(v) for v in CI.C13.reshape(-1)] and len(got) == 64
    assert got[:8] == [2896] * 8 and got[8:16] == [4017, 3406, 2276, 799, -799, -2276, -3406, -4017]
    # orthonormal to the table's rounding: C13 . C13^T = 2^26 I within 8 * 4017 (half a unit per entry, 8 entries a row)
    gram = CI.C13 @ CI.C13.T
    assert np.abs(gram - (1 << 26) * np.eye(8, dtype=np.int64)).max() <= 8 * 4017


# ---- the JPEG restatement against Pillow ----------------------------------------------------------------------------------------
def test_the_jpeg_restatement_against_pillows_round_trip():
    """Per image and quality: the mean absolute gap between the restatement and Pillow's decoder output (quality q, 4:4:4), in grey
    levels, at most one tenth of Pillow's own mean distortion of that image.  Measured (profiles/corrupt_measure.json): mean gap
    0.018 .. 0.62 levels, largest gap 39 levels (a quantisation rounding flip moves a coefficient by a whole step, up to 255),
    Pillow's own distortion 4.1 .. 26.4 levels, worst ratio 3.6 %."""
    worst = 0.0
    for kind, by_size in CI.pin_images().items():
        for (H, W), u8 in by_size.items():
            x = (u8.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)[None]
            for q in (25, 18, 15, 10, 7):
                pil = CI.pillow_jpeg(u8, q).astype(np.int64)
                ours = np.rint(CI.jpeg_q(x, q)[0].transpose(1, 2, 0) * 255).astype(np.int64)
                gap, own = np.abs(ours - pil), float(np.abs(pil - u8.astype(np.int64)).mean())
                print(f"{kind} {H}x{W} q={q}: mean gap {gap.mean():.4f} max gap {int(gap.max())} pillow's distortion {own:.3f} "
                      f"ratio {gap.mean() / own:.4f}")
                worst = max(worst, float(gap.mean()) / own)
                assert float(gap.mean()) <= 0.1 * own, (kind, H, W, q)
    print(f"worst ratio {worst:.4f}")


def test_the_jpeg_restatement_by_hand():
    """A constant grey block has only a DC coefficient, and a grey that is a multiple of the DC step comes back exactly: DC of a
    block of value v is 8 (v - 128); at quality 50 the luminance DC step is 16, so v = 128 + 2 k returns v."""
    for v in (128, 130, 64, 254, 0):
        x = np.full((1, 3, 8, 8), np.float32(v) / np.float32(255), np.float32)
        out = np.rint(CI.jpeg_q(x, 50) * 255).astype(int)
        assert (out == v).all(), (v, np.unique(out))
    x = CI.images(2, 9, 17, seed=3)
    out = CI.jpeg_q(x, 7)
    assert out.shape == x.shape and out.dtype == np.float32 and out.min() >= 0 and out.max() <= 1
    assert np.array_equal(out[:1], CI.jpeg_q(x[:1], 7))  # per image
    levels = np.rint(out * 255)
    assert np.array_equal((levels / np.float32(255)).astype(np.float32), out)  # q / 255 exactly


# ---- blur and pixelate ------------------------------------------------------------------------------------------------------------
def _dyadic(B, H, W, seed):
    """Images on the grid k / 256: sums of up to 317 of them are exact in f32, so the order of a sum cannot show."""
    return (np.random.default_rng(seed).integers(0, 257, (B, 3, H, W)).astype(np.float32) / np.float32(256)).astype(np.float32)


@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (33, 31)])
def test_blur_and_pixelate_restatements_keep_constants_and_commute_with_a_flip(H, W):
    """Constants whose partial sums are exact in f32 (0, 1 and dyadic values: n v / n is then v to the bit), and images on the
    grid k / 256 for the flip: a mirrored table visits a row's taps in the opposite order, which only an exact sum cannot see."""
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for v in (0.0, 1.0, 0.5, 0.75, 37 / 256):
        c = np.full((1, 3, H, W), v, np.float32)
        for s in (1, 2, 3, 4, 5):
            assert np.array_equal(bits(CI.defocus_blur(c, s)), bits(c)), ("disk", v, s)
            assert np.array_equal(bits(CI.pixelate(c, s)), bits(c)), ("pixelate", v, s)
            for k in range(8):
                assert np.array_equal(bits(CI.taps_mean(c, CI.line(CI.TABLE["motion_blur"][s - 1], k))), bits(c)), ("line", v, s, k)
    x = _dyadic(2, H, W, seed=H * 100 + W)
    flip = lambda a: a[..., ::-1]
    for s in (1, 2, 3, 4, 5):
        assert np.array_equal(bits(CI.defocus_blur(flip(x), s)), bits(flip(CI.defocus_blur(x, s)))), s  # the disk: dx -> -dx
        L = CI.TABLE["motion_blur"][s - 1]
        for k in range(8):  # the mirror image of direction k is direction (8 - k) % 8; k = 0 and 4 are their own
            mirrored = sorted((dy, -dx) for dy, dx in CI.line(L, k))
            assert mirrored == sorted(CI.line(L, (8 - k) % 8)), (s, k)
            assert np.array_equal(bits(CI.taps_mean(flip(x), CI.line(L, k))), bits(flip(CI.taps_mean(x, CI.line(L, (8 - k) % 8)))))
    for f in (2, 3, 4, 6, 8):  # blocks anchored at (0, 0) mirror onto blocks where f divides the width
        xw = _dyadic(1, H, 3 * f, seed=f)
        assert np.array_equal(bits(CI.pixelate_f(flip(xw), f)), bits(flip(CI.pixelate_f(xw, f)))), f
        means = CI.pixelate_f(xw, f)
        assert all(np.array_equal(means[..., j], means[..., (j // f) * f]) for j in range(3 * f))  # constant within a block


def test_a_pixelate_block_cut_by_the_edge_averages_what_is_in_the_image():
    x = np.arange(3 * 5 * 7, dtype=np.float32).reshape(1, 3, 5, 7) / np.float32(128)
    got = CI.pixelate_f(x, 4)
    for ch in range(3):
        for (r0, r1) in ((0, 4), (4, 5)):
            for (c0, c1) in ((0, 4), (4, 7)):
                acc = np.float32(0)
                for r in range(r0, r1):
                    for c in range(c0, c1):
                        acc = np.float32(acc + x[0, ch, r, c])
                assert (got[0, ch, r0:r1, c0:c1] == np.float32(acc / np.float32((r1 - r0) * (c1 - c0)))).all()


def test_random_words_are_a_function_of_their_indices():
    from sm3hip import corrupt
    ids = np.array([0, 1, 5, 2 ** 32 - 1, 7])
    for name, s in (("motion_blur", 1), ("motion_blur", 5), ("colour_cast", 3)):
        assert np.array_equal(corrupt.case_words(ids, name, s, 9).astype(np.uint64), CI.case_word(ids, name, s, 9))
        assert not np.array_equal(CI.case_word(ids, name, s, 9), CI.case_word(ids, name, s, 10))
        assert not np.array_equal(CI.case_word(ids, name, s, 9), CI.case_word(ids, name, s, 9 + (1 << 32)))  # the key's high word
    dirs = CI.direction(np.arange(64), 3, 0)
    assert set(int(d) for d in dirs) == set(range(8))  # 64 cases reach all 8 directions
    w, _ = CI.element_words([3, 4], 10, "impulse_noise", 2, 5, 0)
    w1, _ = CI.element_words([4], 6, "impulse_noise", 2, 5, 0)
    assert np.array_equal(w[1, :6], w1[0])  # neither the batch nor the image size enters
    assert not np.array_equal(w, CI.element_words([3, 4], 10, "impulse_noise", 2, 5, 1)[0])  # the modality does
    x = CI.images(2, 33, 31, seed=1)
    out = CI.impulse_noise(x, 5, [0, 1])
    frac = float(((out == 0) | (out == 1)).mean()) - float(((x == 0) | (x == 1)).mean())
    assert abs(frac - 0.27 * (1 - 2 / 16)) < 0.03  # p / 2 to each end, of the elements that were not 0 or 1 already
    raw, cl = CI.gaussian_noise(x, 3, [0, 1])
    assert abs(float((raw - x).std()) - 0.18) < 0.01 and cl.min() >= 0 and cl.max() <= 1


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
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
    from sm3hip import corrupt, ops
    assert all(callable(getattr(ops, n)) for n in ("corrupt_pointwise", "corrupt_taps", "corrupt_pixelate", "corrupt_jpeg"))
    assert all(callable(getattr(corrupt, n)) for n in ("apply", "store_corrupted", "predict_split", "robustness_report", "to_csv",
                                                       "add_flags", "check_flags", "stats_line"))
    assert "corrupt.hip" in open(os.path.join(ROOT, "skin-sm3_amd", "csrc", "Makefile")).read()


def _p(v):
    return C.c_void_p(v) if v else C.c_void_p(0)


NULL = C.c_void_p(0)


def _pointwise(lib, x=0x1000, B=2, H=5, W=7, ids=0x2000, op=0, severity=1, param=0.08, seed=5, modality=0, out=0x3000):
    return lib.sm3_corrupt_pointwise(_p(x), B, H, W, _p(ids), op, severity, param, seed, modality, _p(out), NULL)


@pytest.mark.parametrize("kw", [
    dict(x=0), dict(ids=0), dict(out=0), dict(B=0), dict(H=0), dict(W=0), dict(H=-3), dict(op=2), dict(op=-1), dict(op=11),
    dict(severity=0), dict(severity=6), dict(modality=2), dict(modality=-1), dict(param=-0.1), dict(param=1.5),
    dict(param=float("nan")), dict(op=1, param=0.5), dict(op=1, param=2.0 ** 31 + 1), dict(op=10, param=1.01),
    dict(H=2 ** 15, W=2 ** 15)])
def test_pointwise_rejects_bad_arguments_before_any_launch(kw):
    assert _pointwise(_lib(), **kw) == -1, kw


def _taps(lib, x=0x1000, B=2, H=5, W=7, tables=None, counts=(3,), n_tables=None, max_taps=None, index=(0, 0), out=0x3000,
          null=()):
    tables = [[(0, -1), (0, 0), (0, 1)]] if tables is None else tables
    mt = max(len(t) for t in tables) if max_taps is None else max_taps
    flat = np.zeros((len(tables), max(mt, max(len(t) for t in tables), 1), 2), np.int16)
    for i, t in enumerate(tables):
        flat[i, :len(t)] = np.array(t, np.int16).reshape(-1, 2)
    cn, ix = np.array(counts, np.int32), np.array(index, np.int32)
    ptr = lambda a, name: NULL if name in null else C.c_void_p(a.ctypes.data)
    return lib.sm3_corrupt_taps(_p(x), B, H, W, ptr(flat, "tables"), ptr(cn, "counts"), len(tables) if n_tables is None else n_tables,
                                mt, ptr(ix, "index"), _p(out), NULL)


@pytest.mark.parametrize("kw", [
    dict(x=0), dict(out=0), dict(null=("tables",)), dict(null=("counts",)), dict(null=("index",)), dict(B=0, index=()), dict(H=0),
    dict(W=-1), dict(n_tables=0), dict(n_tables=9), dict(max_taps=0), dict(max_taps=337), dict(counts=(0,)), dict(counts=(4,)),
    dict(index=(0, 1)), dict(index=(-1, 0)), dict(tables=[[(0, 11), (0, 0), (0, 1)]]), dict(tables=[[(-11, 0), (0, 0), (0, 1)]]),
    dict(tables=[[(0, 0)] * 200, [(0, 0)] * 200], counts=(200, 200), index=(0, 1))])
def test_taps_rejects_bad_arguments_before_any_launch(kw):
    assert _taps(_lib(), **kw) == -1, kw


@pytest.mark.parametrize("kw", [dict(x=0), dict(out=0), dict(B=0), dict(H=0), dict(W=0), dict(f=0), dict(f=33), dict(f=-2),
                                dict(B=65536)])
def test_pixelate_rejects_bad_arguments_before_any_launch(kw):
    a = dict(x=0x1000, B=2, H=5, W=7, f=2, out=0x3000)
    a.update(kw)
    assert _lib().sm3_corrupt_pixelate(_p(a["x"]), a["B"], a["H"], a["W"], a["f"], _p(a["out"]), NULL) == -1, kw


@pytest.mark.parametrize("kw", [dict(x=0), dict(out=0), dict(B=0), dict(H=0), dict(W=0), dict(quality=0), dict(quality=101),
                                dict(luma=None), dict(chroma=None), dict(luma=[0] + [16] * 63), dict(chroma=[256] + [16] * 63)])
def test_jpeg_rejects_bad_arguments_before_any_launch(kw):
    a = dict(x=0x1000, B=2, H=5, W=7, quality=25, luma=[16] * 64, chroma=[17] * 64, out=0x3000)
    a.update(kw)
    tabs = [None if a[k] is None else np.array(a[k], np.int32) for k in ("luma", "chroma")]
    ptr = [NULL if t is None else C.c_void_p(t.ctypes.data) for t in tabs]
    assert _lib().sm3_corrupt_jpeg(_p(a["x"]), a["B"], a["H"], a["W"], a["quality"], ptr[0], ptr[1], _p(a["out"]), NULL) == -1, kw


# ---- the host half of the module ------------------------------------------------------------------------------------------------
def test_apply_and_predict_split_refuse_on_the_host():
    from sm3hip import corrupt
    x = torch.zeros(2, 3, 5, 7)
    with pytest.raises(ValueError, match="one of"):
        corrupt.apply(x, "fog", 1)
    for s in (0, 6, 1.0, True):
        with pytest.raises(ValueError, match="severity"):
            corrupt.apply(x, "jpeg", s)
    with pytest.raises(ValueError, match="CUDA"):
        corrupt.apply(x, "jpeg", 1)
    for bad in (torch.zeros(2, 1, 5, 7), torch.zeros(3, 5, 7), torch.zeros(2, 3, 5, 7, dtype=torch.float64), torch.zeros(0, 3, 5, 7)):
        with pytest.raises(ValueError, match="x01"):
            corrupt.apply(bad, "jpeg", 1)
    with pytest.raises(ValueError, match="one of"):
        corrupt.predict_split(None, None, None, 32, [0] * 3, [1] * 3, corruptions=["jpeg", "snow"])
    with pytest.raises(ValueError, match="severities"):
        corrupt.predict_split(None, None, None, 32, [0] * 3, [1] * 3, severities=[1, 7])
    with pytest.raises(ValueError, match="modality"):
        corrupt.predict_split(None, None, None, 32, [0] * 3, [1] * 3, modality="clinical")
    with pytest.raises(ValueError, match="batch_size"):
        corrupt.predict_split(None, None, None, 32, [0] * 3, [1] * 3, batch_size=0)
    assert corrupt._names("all", "t") == CI.NAMES and corrupt._names(["jpeg", "gaussian_noise"], "t") == ["gaussian_noise", "jpeg"]


# ---- the flags ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    """Anything that reaches for the device fails the test."""
    def boom(*a, **k):
        raise AssertionError("touched the GPU before refusing")
    monkeypatch.setattr(torch, "Generator", boom)
    monkeypatch.setattr(torch.cuda, "synchronize", boom)
    monkeypatch.setattr(torch.nn.Module, "to", boom)
    from sm3hip import corrupt
    monkeypatch.setattr(corrupt, "predict_split", boom)


REFUSALS = [
    (["--corrupt", "jpeg"], "real data set"),
    (["--corrupt", "all", "--corrupt-severity", "1"], "real data set"),
    (["--corrupt", "fog"], "must be one of"),
    (["--corrupt", "jpeg", "jpeg"], "none twice"),
    (["--corrupt", "jpeg", "--corrupt-severity", "0"], "1 .. 5"),
    (["--corrupt", "jpeg", "--corrupt-severity", "2", "2"], "distinct"),
    (["--corrupt", "jpeg", "--corrupt-seed", "-1"], "corrupt-seed"),
]


@pytest.mark.parametrize("tool", ["backbone_eval", "mlc_eval"])
@pytest.mark.parametrize("argv,msg", REFUSALS)
def test_the_flags_refusals_stop_before_any_kernel(tool, argv, msg, no_gpu, tmp_path):
    mod = _load(f"sm3_corrupt_{tool}_cpu", os.path.join(TOOLS, f"{tool}.py"))
    with pytest.raises(SystemExit, match=msg):
        mod.main(["--data-name", "synthetic", "--data-path", "-"] + argv + ["--log-path", str(tmp_path)])


@pytest.mark.parametrize("tool", ["backbone_eval", "mlc_eval"])
def test_the_parsers_take_the_flags_and_default_to_nothing(tool, capsys):
    mod = _load(f"sm3_corrupt_{tool}_parser", os.path.join(TOOLS, f"{tool}.py"))
    a = mod.get_parser().parse_args(["--data-path", "-", "--data-name", "synthetic"])
    assert (a.corrupt, a.corrupt_severity, a.corrupt_modality, a.corrupt_seed) == (None, [1, 2, 3, 4, 5], "both", 0)
    a = mod.get_parser().parse_args(["--data-path", "-", "--data-name", "synthetic", "--corrupt", "jpeg", "motion_blur",
                                     "--corrupt-severity", "1", "5", "--corrupt-modality", "clinic", "--corrupt-seed", "11"])
    assert (a.corrupt, a.corrupt_severity, a.corrupt_modality, a.corrupt_seed) == (["jpeg", "motion_blur"], [1, 5], "clinic", 11)
    assert not hasattr(mod.get_parser(tta_flags=False).parse_args(["--data-path", "-", "--data-name", "synthetic"]), "corrupt")
    with pytest.raises(SystemExit):
        mod.get_parser().parse_args(["--data-path", "-", "--data-name", "synthetic", "--corrupt-modality", "dermoscopy"])
    capsys.readouterr()
