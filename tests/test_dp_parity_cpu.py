"""The rank half of the teacher-forcing harness (tests/parity_harness.py) on the reference alone: gloo on the CPU, no GPU,
nothing of the library.  tests/test_dp_parity_gpu.py leans on it.

  * the sharded reference is right: standin_run in fp64 as world ranks with all_reduce_sum at every BatchNorm equals ONE
    process that holds all the ranks' images -- block outputs and boundary gradients per shard, running statistics, and the
    parameter gradients summed over the ranks -- to 1e-9, at world 2 (8 + 8 against 16) and world 3 (6 + 6 + 6 against 18);
  * the clean two-rank bf16 stand-in (the restatement chained, 16 images per rank at geometry A) passes check_run under the
    existing limit rule;
  * the harness notices defects of the EXCHANGE: each is seeded into one BatchNorm of one unit of that stand-in through the
    reducer handed to it, on every rank alike and with the collectives of a clean reducer (a defective one discards their
    results: the ranks stay in step), and check_run must report that unit and no other:
      a. the summed sums divided by the local count                           (H.reduce_local_count)
      b. the backward exchange dropped: the gradient of the packed sums local (H.reduce_forward_only)
      c. a downsample BatchNorm's statistics left local beside an exchanged bn3 -- the parked-sums path taken wrongly
                                                                              (H.reduce_nothing)
    The shards differ clearly (other procedural images, another gradient seed: H.rank_inputs).  What catches each defect is
    printed, and stated beside DEFECTS.
"""
import pytest
import torch

import parity_harness as H

GEO_C, GEO_A = H.GEOMETRIES["C"], H.GEOMETRIES["A"]


# ---- the sharded reference against one process with the whole batch ---------------------------------------------------------
def _sharded_rank(rank, world, n):
    import torch.distributed as dist
    dt = torch.float64  # no rounding anywhere: standin_run's stores are the identity for a type that is not 16-bit
    run = H.standin_run("resnet50", dt, n, 1, *GEO_C, rank=rank, world=world, stat_reduce=H.all_reduce_sum)
    full = H.standin_run("resnet50", dt, n * world, 1, *GEO_C, shards=tuple(range(world)))  # no process group involved
    out = {"x": 0.0, "g": 0.0, "stat": 0.0, "grad": 0.0, "differs": 0.0}
    for kind in ("x", "g"):
        for a, b in zip(run["taps"][kind], full["taps"][kind]):
            rows = a.shape[0]
            assert b.shape[0] == rows * world
            out[kind] = max(out[kind], H.rel(a, b[rank * rows:(rank + 1) * rows]))
    # the shards are not copies of each other: rank 0's rows of the whole batch against the next rank's
    rows = run["taps"]["x"][-1].shape[0]
    fx = full["taps"]["x"][-1]
    out["differs"] = H.rel(fx[:rows], fx[rows:2 * rows])
    for k, v in run["bufs"].items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(full["bufs"][k]) == int(run["buf0"][k]) + 1
        else:
            out["stat"] = max(out["stat"], H.rel(v, full["bufs"][k]))
    for n_, g in run["grads"].items():
        g = g.clone()
        dist.all_reduce(g)
        out["grad"] = max(out["grad"], H.rel(g, full["grads"][n_]))
    return out


@pytest.mark.parametrize("world,n", [(2, 8), (3, 6)], ids=["world2-8+8", "world3-6+6+6"])
def test_sharded_fp64_reference_equals_one_process_with_the_whole_batch(world, n):
    group = H.run_rank_group(_sharded_rank, world, [n], start_s=60, case_s=120, threads=4 if world == 2 else 2)
    res = H.group_case(group, 0)
    print(f"\nworld {world}: {res}")
    for r in range(world):
        o = res[r]
        assert o["x"] < 1e-9 and o["g"] < 1e-9 and o["stat"] < 1e-9 and o["grad"] < 1e-9, (r, o)
        assert o["differs"] > 0.1, o


# ---- the two-rank bf16 stand-in: clean, and with a defect of the exchange in one unit ----------------------------------------
# name -> (unit, BatchNorm, reducer).  Measured by this test (resnet50, bf16, 2 ranks x 16 images at 73 x 37; printed below;
# the same tensors on both ranks), against the limits of the rule (bf16: statistics 1e-3, cosine 0.97, rel 0.3, norm ratios
# 2e-3 input / 3e-2 convolution / 5e-2 BatchNorm, output 1.5e-2 / 2e-2, or 3 x the restatement):
#   a. layer2.1.bn2: its running_mean at 1.0 (twice the mean) and running_var at 5.6e-2.  NOTHING ELSE of the unit leaves its
#      limits: bn2's channels are nearly centred, so the defect is close to a uniform scale 1 / sqrt(2) of bn2's output, which
#      bn3 behind conv3 normalises away, forward and backward.  The running statistics are what pins a count here.
#   b. layer4.1.bn1 (96 rows per rank): conv1's weight gradient at cosine 0.956, |norm ratio - 1| 6.2e-2 .. 6.7e-2 (the missing
#      peer sum(dz * xhat) is a multiple of W row by row, the direction the true gradient is orthogonal to), and the unit's
#      input gradient at |norm ratio - 1| 2.6e-3 .. 3.0e-3.
#   c. layer3.0.downsample.1: the block output at 6.6e-2 .. 8.1e-2 (max 0.10 .. 0.12), its running_mean / running_var at 8.4e-2 /
#      2.5e-2, the downsample convolution's weight gradient at cosine 0.82 .. 0.83, the BatchNorm's gamma gradient at 0.18 rel,
#      the input gradient at |norm ratio - 1| 1.7e-2 .. 2.3e-2.
DEFECTS = {
    "clean": None,
    "a-local-count": ("layer2.1.", "bn2", "reduce_local_count"),
    "b-backward-exchange-dropped": ("layer4.1.", "bn1", "reduce_forward_only"),
    "c-downsample-statistics-local": ("layer3.0.", "downsample.1", "reduce_nothing"),
}
STANDIN_CASES = list(DEFECTS)


def _standin_rank(rank, world, name):
    d = DEFECTS[name]
    defects = {d[0]: {"reduce": {d[1]: getattr(H, d[2])}}} if d else None
    run = H.standin_run("resnet50", torch.bfloat16, 16, 1, *GEO_A, defects=defects, rank=rank, world=world,
                        stat_reduce=H.all_reduce_sum)
    _, _, fails = H.check_run(run, f"cpu-dp-standin-{name}-rank{rank}", stat_reduce=H.all_reduce_sum)
    return [[str(f[0]), str(f[1])] + [float(v) for v in f[2:]] for f in fails]


@pytest.fixture(scope="module")
def standin_group():
    return H.run_rank_group(_standin_rank, 2, STANDIN_CASES, start_s=60, case_s=300)


@pytest.mark.parametrize("name", STANDIN_CASES)
def test_exchange_defects_fail_their_own_unit_only_and_the_clean_stand_in_passes(standin_group, name):
    res = H.group_case(standin_group, STANDIN_CASES.index(name))
    if DEFECTS[name] is None:
        for r in (0, 1):
            assert not res[r], (r, res[r][:8])
        return
    unit = DEFECTS[name][0]
    for r in (0, 1):
        mine = [f for f in res[r] if f[0].startswith(unit)]
        print(f"\n{name}, rank {r}: {mine[:6]}")
        assert mine, f"{name} in {unit} went unnoticed on rank {r}"
        assert len(mine) == len(res[r]), [f for f in res[r] if not f[0].startswith(unit)][:8]
