"""Every block of the 16-bit TRAINING step against fp64, at the benchmarked shapes, by teacher forcing.

The whole-encoder comparisons (tests/test_round5_gpu.py, tests/test_config_gpu.py) cannot pin a train-mode gradient: 53
train-mode BatchNorms amplify rounding to O(1) direction errors at random init, so their bf16 floors pass almost anything.
Here each unit -- the stem (7x7/2 conv, BatchNorm, ReLU, max-pool) and each of the 16 Bottlenecks -- is checked ON ITS
OWN: the engine runs one train-mode forward and backward with block-boundary taps (SM3Engine.encoder_forward /
encoder_backward, taps=), and each unit is recomputed in fp64 on the GPU from the engine's OWN input to that unit and the
engine's OWN upstream gradient.  Every unit is then well conditioned, and per tensor it is compared:

  * the output (relative L2 error, max error over the tensor's max),
  * running_mean / running_var of every BatchNorm (relative L2) and num_batches_tracked (exactly),
  * the gradient of every parameter tensor -- conv weights, BatchNorm gamma / beta -- (cosine, relative L2),
  * the gradient at the unit's input, i.e. the engine's next tap down (cosine, relative L2).

At 224 x 224 and B = 256 pairs, layer 1 has 1.6 M rows per view: the size-selected paths (slab counts of the fixed-order
weight gradients, the eight-lane linbn_moments, view tiles, the stride-2 join, bn3's statistics by linearity from fp32
Gram matrices) run exactly as bench.py runs them.

The fp64 reference is oracle/sm3_oracle.py's `batchnorm` (one call per view half, in view order: statistics per view and
the two running-statistic updates) around fp64 convolutions written as one matmul per filter tap over NHWC rows (Conv):
no unfold matrix, and weight gradients split over images so that no GEMM has a 1.6 M-long K loop on a handful of tiles.

The engine run, the fp64 units, the metrics and the per-unit comparison live in tests/parity_harness.py, which takes any
H x W (taps are reshaped with explicit map sizes).  This file keeps the cases at the benchmarked shapes and BOUNDS, the table
measured there.  Geometry coverage -- odd, non-square and tiny images, every block family, limits of
max(BOUNDS, 3 x the mode restatement's own error) -- lives in tests/test_geometry_parity_gpu.py, and the reference-only floors
behind those limits in tests/test_parity_harness_cpu.py.
"""
import pytest
import torch

import parity_harness as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


CASES = {  # dtype, images (both views), views, size
    "bf16-2x256-224": (torch.bfloat16, 512, 2, 224),   # exactly what bench.py times
    "f16-2x256-224": (torch.float16, 512, 2, 224),     # the --amp recipe, same kernel templates
    "bf16-16-224": (torch.bfloat16, 16, 1, 224),       # unpaired: no view tiles, stride-2 join without the 256 multiple
    "f32-16-224": (torch.float32, 16, 1, 224),         # exact-f32 mode: two-pass BatchNorms, f32 MFMA
    "f16-2x128-448": (torch.float16, 256, 2, 448),     # BASELINE config 5: the largest tensors
}


@pytest.mark.parametrize("case", list(CASES))
def test_every_block_of_the_train_step_against_fp64_by_teacher_forcing(case):
    dt, N, V, size = CASES[case]
    run = H.engine_run("resnet50", dt, N, V, size, size, DEV)
    assert len(run["taps"]["x"]) == len(run["taps"]["g"]) == len(run["plan"].blocks) + 1 == 17
    # the stem (conv 7x7/2 + bn1 + ReLU + max-pool on the images as the engine saw them; no input gradient), then the
    # Bottlenecks, each from the engine's own input and upstream gradient, with this file's bounds alone
    rep, _, fails = H.check_run(run, case, base=BOUNDS[H.DTNAME[dt]], restate=False)
    H.report(case, rep)
    assert not fails, fails[:8]


# Measured (MI355X, det mode: the same bits on every run), worst tensor over all units and the cases of a mode:
#   bf16 (2x256 and 16 images at 224): output rel 5.7e-3, max 7.5e-3; running statistics 2.5e-4; gradient cosine 0.99463,
#        rel 0.104; |norm ratio - 1| of the unit's input gradient 3.0e-4, of a conv weight gradient 8.1e-3, of a BatchNorm
#        parameter gradient 1.4e-2
#   f16 (2x256 at 224, 2x128 at 448): output 7.2e-4, max 8.9e-4; statistics 1.2e-5; cosine 0.99953, rel 3.1e-2; ratios 1.7e-5
#        (input), 1.2e-3 (conv), 9.4e-3 (BatchNorm)
#   f32 (16 images at 224): output 1.2e-6, max 1.4e-6; statistics 1.1e-7; cosine 0.999996, rel 2.8e-3; ratios 1.9e-6, 2.0e-5,
#        2.2e-4
# The 16-bit gradient errors are far above 2^-8: the engine's saved activations and gradients are 16-bit, and a gradient
# behind a train-mode BatchNorm is a cancellation -- d(beta) = sum(dz) of a dz whose mean the next BatchNorm removed,
# d(W) of a conv feeding a BatchNorm orthogonal to W row by row -- which turns per-element rounding into a relative error
# of 1e-2 .. 1e-1 in the tensor (bf16 / f16 = 3.3 in every stage, the same for paired and unpaired batches: no single block
# stands out).  That noise is nearly orthogonal to the gradient, so a gradient's NORM stays within 3e-4 (bf16) of fp64:
# the norm ratio of the input gradient is the sharp check of the backward pass -- one linbn coefficient scaled by 1 + 1e-2
# moves it to 1.0e-2 in every block while the cosines do not move; a dropped stride-2 join addend drops the cosine of the
# stage's input gradient to 0.82; view-1 tiles of the fused conv3 epilogue using view 0's BatchNorm triple the max output
# error (2.8e-2 .. 3.8e-2).  In f32 every tensor is at 1e-6 except a few in three blocks (layer2.1, layer2.3, layer4.2:
# conv1 / conv2 weights and bn1 / bn2 bias at 4e-4 .. 2.8e-3, their gamma at 1e-6): a bn1 / bn2 output within rounding of 0
# takes the other side of the ReLU than in fp64 -- beta = 0, so it moves sum(dz) and not sum(dz * xhat) -- and over the
# 784 .. 12 544 rows of those maps one element is 1e-3 of a cancelled sum.  Bounds: 3 - 7x the measured values.
BOUNDS = {
    "bf16": {"out_rel": 1.5e-2, "out_max": 2e-2, "stat_rel": 1e-3, "cos": 0.97, "rel": 0.3,
             "in_ratio": 2e-3, "conv_ratio": 3e-2, "bn_ratio": 5e-2},
    "f16": {"out_rel": 3e-3, "out_max": 3e-3, "stat_rel": 6e-5, "cos": 0.9975, "rel": 0.1,
            "in_ratio": 1e-4, "conv_ratio": 6e-3, "bn_ratio": 3e-2},
    "f32": {"out_rel": 5e-6, "out_max": 6e-6, "stat_rel": 5e-7, "cos": 0.99998, "rel": 1e-2,
            "in_ratio": 1e-5, "conv_ratio": 1e-4, "bn_ratio": 1e-3},
}
