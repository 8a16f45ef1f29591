"""GPU: the colour, finish and crop kernels of csrc/augment.hip called directly, against oracle/augment_oracle.py in fp64
on the same fp32 values.

Pixels (tests/edge_inputs.py pixel_table): the 6^3 combinations of {0, 1/255, 127/255, 128/255, 254/255, 1} -- every cube
corner, grey ramp and channel tie -- near-ties down to one ulp in all arrangements, and 3000 random pixels, laid out as
61 x 54 (no multiple of 64 or 256), 7 x 9 (less than one wave), 33 x 31 (1023) and 25 x 41 (1025 pixels: one more than
the mean kernel's block).  Bounds: 1e-5 per colour op, 2e-5 per chain of four, on [0, 1] values, no pixel excluded (the hue
round trip is continuous); tests/test_edge_refs_cpu.py shows the oracle in fp32 within a quarter of them.  The contrast
mean: 2e-7.  The finish kernel: 5e-5 on the normalised output (1e-5 over the smallest std).  Crops: 1e-5 on every pixel."""
import ctypes as C

import pytest
import torch

import edge_inputs as E
from oracle import augment_oracle as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from sm3hip import _lib
    return _lib


def _color_op(img, ops, factors):
    """sm3_aug_color_op in place on img [B, 3, H, W]; -> the gray_mean buffer (means of the images as they came in)"""
    from sm3hip import ops as O
    lib = _lib()
    B, _, H, W = img.shape
    opd = torch.as_tensor(ops, dtype=torch.int32).contiguous().to(DEV)
    fd = torch.as_tensor(factors, dtype=torch.float32).contiguous().to(DEV)
    gm = torch.full((B,), float("nan"), device=DEV)
    lib.check(lib.load().sm3_aug_color_op(O._ptr(img), B, H, W, O._ptr(opd), O._ptr(fd), O._ptr(gm), O._stream()),
              "sm3_aug_color_op")
    torch.cuda.synchronize()
    return gm.cpu()


def _finish(img, gray, sigma, mean, std):
    from sm3hip import ops as O
    lib = _lib()
    B, _, H, W = img.shape
    gd = torch.as_tensor(gray, dtype=torch.uint8).to(DEV)
    sd = torch.as_tensor(sigma, dtype=torch.float32).to(DEV)
    out = torch.full_like(img, float("nan"))
    m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    lib.check(lib.load().sm3_aug_finish(O._ptr(img), B, H, W, O._ptr(gd), O._ptr(sd), m3, s3, O._ptr(out), O._stream()),
              "sm3_aug_finish")
    torch.cuda.synchronize()
    return out.cpu()


_refs = {}


def _ref(size, op, f):
    """fp64 reference of one op on the table images of one size: computed once, shared, never written to."""
    key = (size, op, f)
    if key not in _refs:
        _refs[key] = E.color_ref(E.table_images(*size), op, f)
    return _refs[key]


@pytest.mark.parametrize("size", E.AUG_SIZES, ids=str)
@pytest.mark.parametrize("op", [1, 2, 3, 4], ids=["brightness", "contrast", "saturation", "hue"])
def test_colour_op_on_the_pixel_table(op, size):
    src = E.table_images(*size)
    B = src.shape[0]
    worst = 0.0
    for f in E.AUG_FACTORS[op]:
        img = src.to(DEV)
        _color_op(img, [op] * B, [f] * B)
        got = img.cpu()
        assert bool(torch.isfinite(got).all())
        worst = max(worst, float((got.double() - _ref(size, op, f)).abs().max()))
        if op != 4 and f == 1.0:  # factor 1 is the identity: f x + (1 - f) m = x exactly
            assert torch.equal(got.view(torch.int32), src.view(torch.int32)), (op, size)
    name = {1: "brightness", 2: "contrast", 3: "saturation", 4: "hue"}[op]
    assert E.record(f"colour op: {name}", worst, E.AUG_OP_LIMIT) <= 1.0, (op, size, worst)


@pytest.mark.parametrize("size", E.AUG_SIZES, ids=str)
def test_contrast_mean_of_the_grey_image(size):
    src = E.table_images(*size)
    B = src.shape[0]
    gm = _color_op(src.to(DEV), [2] * B, [0.7] * B)
    want = torch.stack([A.gray(src[b].double()).mean() for b in range(B)])
    err = float((gm.double() - want).abs().max())
    assert E.record("contrast: mean of the grey image", err, E.AUG_MEAN_LIMIT) <= 1.0, (size, err)


@pytest.mark.parametrize("size", E.AUG_SIZES, ids=str)
def test_samples_of_one_launch_carry_different_ops(size):
    """op 0 .. 4 side by side in one batch: op 0 leaves its sample untouched bit for bit, the others get their own op."""
    src = E.table_images(*size, B=10, seed=4)
    ops = [0, 1, 2, 3, 4, 0, 4, 3, 2, 1]
    fac = [0.3, 0.2, 1.8, 0.0, -0.2, 1.7, 1.0 / 3, 1.8, 0.2, 1.8]
    img = src.to(DEV)
    _color_op(img, ops, fac)
    got = img.cpu()
    worst = 0.0
    for b, (op, f) in enumerate(zip(ops, fac)):
        if op == 0:
            assert torch.equal(got[b].view(torch.int32), src[b].view(torch.int32)), b
        else:
            worst = max(worst, float((got[b].double() - A.color_op(src[b].double(), op, E.f32(f))).abs().max()))
    assert E.record("colour op: mixed ops in one launch", worst, E.AUG_OP_LIMIT) <= 1.0, worst


def test_fifty_random_chains_of_four_ops():
    ops, fac = E.draw_chains(50, seed=50)
    src = E.table_images(61, 54, B=50, seed=9)
    img = src.to(DEV)
    for pos in range(4):
        _color_op(img, ops[pos], fac[pos])
    err = float((img.cpu().double() - E.chain_ref(src, ops, fac)).abs().max())
    assert E.record("colour chain of four ops", err, E.AUG_CHAIN_LIMIT) <= 1.0, err


FINISH_SIZES = [(2, 2), (2, 17), (17, 2), (61, 54)]
FINISH_GRAY = [0, 0, 0, 0, 1, 1, 1, 1]
FINISH_SIGMA = [0.0, 0.1, 0.7, 2.0, 0.0, 0.1, 0.7, 2.0]


@pytest.mark.parametrize("size", FINISH_SIZES, ids=str)
def test_finish_kernel_grey_blur_normalize(size):
    """Every grey x sigma combination as the samples of one launch (reflect edges: every pixel of the small sizes); a
    sample launched alone gives the same bits, so no parameter leaks between samples."""
    src = E.table_images(*size, B=8, seed=6)
    img = src.to(DEV)
    got = _finish(img, FINISH_GRAY, FINISH_SIGMA, E.MEAN, E.STD)
    err = float((got.double() - E.finish_ref(src, FINISH_GRAY, FINISH_SIGMA, E.MEAN, E.STD)).abs().max())
    assert E.record("finish: grey, blur, normalize", err, E.AUG_FINISH_LIMIT) <= 1.0, (size, err)
    for b in range(8):
        alone = _finish(img[b:b + 1].contiguous(), FINISH_GRAY[b:b + 1], FINISH_SIGMA[b:b + 1], E.MEAN, E.STD)
        assert torch.equal(alone[0].view(torch.int32), got[b].view(torch.int32)), b


@pytest.mark.parametrize("size", FINISH_SIZES, ids=str)
def test_finish_kernel_keeps_a_constant_image_constant(size):
    """The blur weights sum to 1."""
    H, W = size
    levels = torch.tensor([0.0, 1.0 / 255, 0.3, 0.5, 0.7, 254.0 / 255, 1.0, 0.123])
    src = levels.view(8, 1, 1, 1).expand(8, 3, H, W).contiguous()
    got = _finish(src.to(DEV), FINISH_GRAY, FINISH_SIGMA, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)).double()
    worst = 0.0
    for b in range(8):
        want = float(levels[b].double()) * ((0.2989 + 0.587 + 0.114) if FINISH_GRAY[b] else 1.0)
        worst = max(worst, float((got[b] - want).abs().max()))
    assert E.record("finish: constant image", worst, 1e-6) <= 1.0, worst


def _crop_cases():
    Hs, Ws = 150, 210
    small = [("1x1 box", (70, 99, 1, 1)), ("1x1 box in the last corner", (Hs - 1, Ws - 1, 1, 1)),
             ("one-row box", (33, 20, 1, 57)), ("one-column box", (20, 33, 57, 1)),
             ("box flush with the bottom-right corner", (Hs - 40, Ws - 56, 40, 56))]
    return Hs, Ws, [(name, box, (16, 16)) for name, box in small] + [("whole image down to 8 x 8", (0, 0, Hs, Ws), (8, 8))]


@pytest.mark.parametrize("which", range(6), ids=["1x1", "1x1-corner", "row", "column", "flush", "whole"])
def test_crop_edges_fixed_and_ragged(which):
    from sm3hip import ops as O
    lib = _lib()
    Hs, Ws, cases = _crop_cases()
    name, box, (H, W) = cases[which]
    src = torch.randint(0, 256, (Hs, Ws, 3), generator=torch.Generator().manual_seed(150), dtype=torch.uint8)
    boxes = torch.tensor([box, box], dtype=torch.int32)
    flips = torch.tensor([0, 1], dtype=torch.uint8)
    srcd = src.unsqueeze(0).expand(2, -1, -1, -1).contiguous().to(DEV)
    bd, fd = boxes.to(DEV), flips.to(DEV)
    fixed = torch.full((2, 3, H, W), float("nan"), device=DEV)
    lib.check(lib.load().sm3_aug_resized_crop(O._ptr(srcd), 2, Hs, Ws, O._ptr(bd), O._ptr(fd), O._ptr(fixed), H, W, O._stream()),
              "sm3_aug_resized_crop")
    arena = src.reshape(-1).to(DEV)
    off, hh, ww = torch.zeros(1, dtype=torch.int64), torch.tensor([Hs], dtype=torch.int32), torch.tensor([Ws], dtype=torch.int32)
    index = torch.zeros(2, dtype=torch.int32)
    ragged = torch.full((2, 3, H, W), float("nan"), device=DEV)
    lib.check(lib.load().sm3_aug_resized_crop_ragged(O._ptr(arena), arena.numel(), off.data_ptr(), hh.data_ptr(), ww.data_ptr(),
                                                     1, index.data_ptr(), boxes.data_ptr(), flips.data_ptr(), 2, O._ptr(ragged),
                                                     H, W, O._stream()), "sm3_aug_resized_crop_ragged")
    torch.cuda.synchronize()
    assert torch.equal(fixed.view(torch.int32), ragged.view(torch.int32)), name
    got = fixed.cpu().double()
    worst = 0.0
    for b in range(2):
        want = A.resized_crop(src, box, bool(flips[b]), H, W)
        worst = max(worst, float((got[b] - want).abs().max()))
        if box[2] == 1 and box[3] == 1:  # a 1 x 1 box up-scaled: every output pixel is that pixel
            px = src[box[0], box[1]].double().view(3, 1, 1) / 255.0
            assert float((got[b] - px).abs().max()) <= 1e-6, name
    assert E.record("resized crop at box edges", worst, 1e-5) <= 1.0, (name, worst)
