"""Inputs and numpy restatements for the corruption tests (tests/test_corrupt_cpu.py, tests/test_corrupt_gpu.py): every corruption
of sm3hip/corrupt.py written again from that module's text alone -- its own Philox, its own tap lists, its own quantisation
tables -- with every f32 operation rounded on its own.  Images are numpy float32 [B, 3, H, W] in [0, 1].  Nothing here touches a
device or imports the package."""
import io
import math

import numpy as np

F32 = np.float32
NAMES = ["gaussian_noise", "impulse_noise", "defocus_blur", "motion_blur", "pixelate", "jpeg", "darken", "brighten", "contrast",
         "desaturate", "colour_cast"]
CODE = {n: i for i, n in enumerate(NAMES)}
TABLE = {"gaussian_noise": (0.08, 0.12, 0.18, 0.26, 0.38), "impulse_noise": (0.03, 0.06, 0.09, 0.17, 0.27),
         "defocus_blur": (3, 4, 6, 8, 10), "motion_blur": (5, 9, 13, 17, 21), "pixelate": (2, 3, 4, 6, 8), "jpeg": (25, 18, 15, 10, 7),
         "darken": (0.8, 0.65, 0.5, 0.35, 0.2), "brighten": (1.2, 1.4, 1.6, 1.8, 2.0), "contrast": (0.75, 0.6, 0.45, 0.3, 0.15),
         "desaturate": (0.8, 0.6, 0.4, 0.2, 0.0), "colour_cast": (0.05, 0.1, 0.15, 0.2, 0.3)}
SHAPES = [(1, 1, 1), (2, 5, 7), (1, 8, 8), (2, 9, 17), (1, 16, 24), (1, 33, 31), (1, 70, 70)]  # (B, H, W) of the GPU tests
ALL_SEVERITIES_AT = (2, 9, 17)


def images(B, H, W, seed=0):
    """Seeded [B, 3, H, W] float32 in [0, 1] with exact 0 and 1 values among them."""
    g = np.random.default_rng(seed * 7919 + B * 10007 + H * 101 + W)
    x = g.random((B, 3, H, W), dtype=np.float32)
    flat = x.reshape(-1)
    pick = g.permutation(flat.size)
    flat[pick[:max(1, flat.size // 16)]] = 0.0
    flat[pick[-max(1, flat.size // 16):]] = 1.0
    if flat.size == 3:
        flat[:] = [0.0, 0.37, 1.0]
    return x


def clamp01(v):
    return np.minimum(np.maximum(v, F32(0)), F32(1)).astype(F32)


# ---- randomness -------------------------------------------------------------------------------------------------------------
def philox(c0, c1, c2, c3, seed):
    """Philox4x32-10 (Salmon et al., SC 2011), key = the 64-bit seed, low word first; uint64 arrays of 32-bit words -> 4 words."""
    m = np.uint64(0xFFFFFFFF)
    c = [np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def case_word(ids, name, severity, seed):
    """uint64 [B]: word 0 at counter (0xFFFFFFFF, case, code << 8 | severity, 7)."""
    ids = np.asarray(ids, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    return philox(np.uint64(0xFFFFFFFF), ids, np.uint64(CODE[name] << 8 | severity), np.uint64(7), seed)[0]


def element_words(ids, E, name, severity, seed, modality):
    """uint64 [B, E]: element e takes word e % 4 at counter (e / 4, case, modality << 16 | code << 8 | severity, 7); also the
    four words per call [4][B, ceil(E / 4)] for the normals."""
    ids = (np.asarray(ids, dtype=np.uint64) & np.uint64(0xFFFFFFFF))[:, None]
    e4 = np.arange((E + 3) // 4, dtype=np.uint64)[None, :]
    w = philox(e4, ids, np.uint64(modality << 16 | CODE[name] << 8 | severity), np.uint64(7), seed)
    return np.stack(w, axis=2).reshape(ids.shape[0], -1)[:, :E], w


def gaussian_noise(x, severity, ids, seed=0, modality=0):
    """(before the clamp, after it): fadd(x, fmul(sigma, z)), z by float64 Box-Muller on the word pairs, rounded to f32 once."""
    B, E = x.shape[0], x[0].size
    _, w = element_words(ids, E, "gaussian_noise", severity, seed, modality)
    u = [(v.astype(np.float64) + 0.5) * 2.0 ** -32 for v in w]
    z = np.empty(w[0].shape + (4,), F32)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[a]))
        z[..., a] = (r * np.cos(2.0 * np.pi * u[a + 1])).astype(F32)
        z[..., a + 1] = (r * np.sin(2.0 * np.pi * u[a + 1])).astype(F32)
    z = z.reshape(B, -1)[:, :E].reshape(x.shape)
    raw = (x + (F32(TABLE["gaussian_noise"][severity - 1]) * z).astype(F32)).astype(F32)
    return raw, clamp01(raw)


def impulse_noise(x, severity, ids, seed=0, modality=0):
    T = int(TABLE["impulse_noise"][severity - 1] * 2 ** 31)
    w, _ = element_words(ids, x[0].size, "impulse_noise", severity, seed, modality)
    w = w.reshape(x.shape)
    out = x.copy()
    out[w < np.uint64(T)] = 0.0
    out[w >= np.uint64(2 ** 32 - T)] = 1.0
    return out


def colour_cast(x, severity, ids, seed=0):
    c = F32(TABLE["colour_cast"][severity - 1])
    hi, lo = F32(1) + c, F32(1) - c
    cool = (case_word(ids, "colour_cast", severity, seed) & np.uint64(1)).astype(bool)
    g = np.where(cool[:, None], np.array([lo, F32(1), hi], F32)[None], np.array([hi, F32(1), lo], F32)[None]).astype(F32)
    return clamp01((x * g[:, :, None, None]).astype(F32))


# ---- blurs and pixelate -----------------------------------------------------------------------------------------------------
def disk(r):
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r * r]


def line(L, k):
    th = k * math.pi / 8
    return [(round(t * math.sin(th)), round(t * math.cos(th))) for t in range(-(L - 1) // 2, (L - 1) // 2 + 1)]


def direction(ids, severity, seed):
    return (case_word(ids, "motion_blur", severity, seed) & np.uint64(7)).astype(np.int64)


def taps_mean(x, taps):
    """One image batch x [..., H, W] under one tap list: the sum in list order from 0, every add rounded, clamped coordinates, one
    division by the tap count."""
    H, W = x.shape[-2:]
    yy, xx = np.arange(H)[:, None], np.arange(W)[None, :]
    acc = np.zeros(x.shape, F32)
    for dy, dx in taps:
        acc = (acc + x[..., np.clip(yy + dy, 0, H - 1), np.clip(xx + dx, 0, W - 1)]).astype(F32)
    return (acc / F32(len(taps))).astype(F32)


def defocus_blur(x, severity):
    return taps_mean(x, disk(TABLE["defocus_blur"][severity - 1]))


def motion_blur(x, severity, ids, seed=0):
    ks = direction(ids, severity, seed)
    return np.stack([taps_mean(x[b], line(TABLE["motion_blur"][severity - 1], int(ks[b]))) for b in range(x.shape[0])])


def pixelate_f(x, f):
    """Blocks anchored at (0, 0); a block's in-image pixels added row-major from 0, every add rounded, one division by their number."""
    H, W = x.shape[-2:]
    nby, nbx = -(-H // f), -(-W // f)
    acc, cnt = np.zeros(x.shape[:-2] + (nby, nbx), F32), np.zeros((nby, nbx), np.int64)
    for dr in range(f):
        for dc in range(f):
            rows, cols = np.arange(nby) * f + dr, np.arange(nbx) * f + dc
            vr, vc = rows < H, cols < W
            sub = x[..., rows[vr][:, None], cols[vc][None, :]]
            a = acc[..., :int(vr.sum()), :int(vc.sum())]  # the in-image rows and columns are a leading run
            acc[..., :int(vr.sum()), :int(vc.sum())] = (a + sub).astype(F32)
            cnt[:int(vr.sum()), :int(vc.sum())] += 1
    mean = (acc / cnt.astype(F32)).astype(F32)
    return mean[..., (np.arange(H) // f)[:, None], (np.arange(W) // f)[None, :]]


def pixelate(x, severity):
    return pixelate_f(x, TABLE["pixelate"][severity - 1])


# ---- JPEG -------------------------------------------------------------------------------------------------------------------
K1 = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
      103, 99]
K2 = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + \
    [99] * 32
C13 = np.array([[int(np.rint(2 ** 13 * (math.sqrt(1 / 8) if k == 0 else math.sqrt(2 / 8)) * math.cos((2 * n + 1) * k * math.pi / 16)))
                 for n in range(8)] for k in range(8)], dtype=np.int64)


def quant(quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.array([min(max((b * s + 50) // 100, 1), 255) for b in base], dtype=np.int64).reshape(8, 8) for base in (K1, K2)]


def jpeg_q(x, quality):
    """The integer 4:4:4 round trip of x [B, 3, H, W] at a quality, as the module text numbers its steps."""
    B, _, H, W = x.shape
    q8 = np.clip(np.rint((x * F32(255)).astype(F32)), 0, 255).astype(np.int64)                                  # 1
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    q8 = q8[:, :, np.minimum(np.arange(Hp), H - 1)[:, None], np.minimum(np.arange(Wp), W - 1)[None, :]]       # edge-replicated
    R, G, Bl = q8[:, 0], q8[:, 1], q8[:, 2]
    ycc = [(19595 * R + 38470 * G + 7471 * Bl + 32768) >> 16,                                                    # 2
           (-11059 * R - 21709 * G + 32768 * Bl + (128 << 16) + 32767) >> 16,
           (32768 * R - 27439 * G - 5329 * Bl + (128 << 16) + 32767) >> 16]
    tables, back = quant(quality), []
    for ch, plane in enumerate(ycc):
        X = plane.reshape(B, Hp // 8, 8, Wp // 8, 8).transpose(0, 1, 3, 2, 4) - 128                            # [B, by, bx, 8, 8]
        Fq = np.einsum("km,...mn,ln->...kl", C13, X, C13)                                                       # 3
        t = tables[1 if ch else 0]                                                                              # 4
        d = t << 26
        qv = np.sign(Fq) * ((2 * np.abs(Fq) + d) // (2 * d))                                                    # 5
        y = (np.einsum("km,...kl,ln->...mn", C13, qv * t, C13) + (1 << 25)) >> 26                                # 6
        back.append(np.clip(y + 128, 0, 255).transpose(0, 1, 3, 2, 4).reshape(B, Hp, Wp)[:, :H, :W])
    Y, cb, cr = back[0], back[1] - 128, back[2] - 128                                                            # 7
    rgb = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                    Y + ((116130 * cb + 32768) >> 16)], axis=1)
    return (np.clip(rgb, 0, 255).astype(F32) / F32(255)).astype(F32)


def jpeg(x, severity):
    return jpeg_q(x, TABLE["jpeg"][severity - 1])


def pillow_jpeg(u8, quality):
    """Pillow's own round trip of one uint8 [H, W, 3] image: quality, 4:4:4."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(u8, "RGB").save(buf, "JPEG", quality=quality, subsampling=0)
    return np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))


def pin_images():
    """{"smooth" | "textured": {(H, W): uint8 [H, W, 3]}} at 73 x 37 and 64 x 64, seeded."""
    out = {"smooth": {}, "textured": {}}
    for H, W in ((73, 37), (64, 64)):
        g = np.random.default_rng(H * 1000 + W)
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        smooth = np.stack([0.5 + 0.4 * np.sin(yy / 11.0 + p) * np.cos(xx / 7.0 - p) + 0.1 * (xx + yy) / (H + W) - 0.05
                           for p in (0.0, 1.0, 2.0)], axis=2)
        out["smooth"][(H, W)] = np.clip(np.rint(smooth * 255), 0, 255).astype(np.uint8)
        tex = 0.5 * smooth + 0.5 * g.random((H, W, 3)) * (((yy // 5 + xx // 3) % 2)[:, :, None] * 0.8 + 0.2)
        out["textured"][(H, W)] = np.clip(np.rint(tex * 255), 0, 255).astype(np.uint8)
    return out


def corrupt(x, name, severity, ids, seed=0, modality=0):
    """The restatement of the seven corruptions that have new device code, by name."""
    if name == "gaussian_noise":
        return gaussian_noise(x, severity, ids, seed, modality)[1]
    if name == "impulse_noise":
        return impulse_noise(x, severity, ids, seed, modality)
    if name == "colour_cast":
        return colour_cast(x, severity, ids, seed)
    if name == "motion_blur":
        return motion_blur(x, severity, ids, seed)
    return {"defocus_blur": defocus_blur, "pixelate": pixelate, "jpeg": jpeg}[name](x, severity)
