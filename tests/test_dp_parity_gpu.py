"""Every block of the SYNCHRONISED-BatchNorm training step against fp64, by teacher forcing with real ranks (GPU).

The data-parallel form of the encoder step runs code that no single-rank test reaches: with SM3Engine.stat_sync set, conv_bn
takes the global count and the parked-sums path (one exchange for the downsample BatchNorm and bn3), _bn_backward_sums and
bn_backward_join exchange a copy of their sums, conv3_bn3_fused and join_fused fold their partial rows before the exchange,
and conv3_backward_linbn recomputes its coefficients from the exchanged sums (sm3_linbn_coef, launched nowhere else).  Which
slice of which buffer is exchanged, which count divides which sum, which unit is finalised after which exchange: here every
stem, Bottleneck and BasicBlock of rank r's step is recomputed in fp64 from the engine's own input and own upstream gradient
with SyncBatchNorm's semantics (tests/parity_harness.py: check_run(stat_reduce=all_reduce_sum); tests/test_dp_parity_cpu.py
shows that this reference equals one process with the whole batch, and that it notices a local count, a dropped backward
exchange and un-exchanged downsample statistics).  Limits: the existing rule, max(BOUNDS[mode], 3 x the restatement on the
same unit); no limit comes from the engine, none is loosened.

The ranks are processes on the one GPU over gloo, ONE spawn per world size (two groups, at most three processes with the GPU
open); a group runs its cases one after the other and each test asserts on its own case.  Every wait has a limit, nothing is
retried: after a failure the rest of the group's cases fail with its report.

CASES -- the smallest per-rank shapes at which each synchronised branch runs -- and, per case, the forms its blocks must
have taken (the plan's own records; a knob that silently selected another form fails), the views that ran, equal weights on
all ranks.  One case also shows that the peer's statistics did enter: rank 0's block outputs differ from a single-rank run on
the same images by more than the mode's out_rel bound.  profiles/dp_parity_measure.md holds the measured values.
"""
import hashlib
import os

import pytest
import torch

import parity_harness as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KNOBS = ("SM3_LINBN", "SM3_LINBN_FWD", "SM3_LINBN_DS", "SM3_LINBN_JOIN", "SM3_PAIR_VIEWS")  # what selects a block's form
# id, arch, mode, world, images per rank (all views), views, (H, W), knobs, the world-1 comparison
CASES = [
    # both views in one batch, the smallest shape pair_ok admits: join_fused, conv3_bn3_fused, linbn_fold, linbn_coef with
    # lin_d, one exchange for both views
    dict(id="resnet50-bf16-w2-2x32-64", arch="resnet50", mode="bf16", world=2, N=64, V=2, hw=(64, 64), env={}),
    # unpaired, an odd side into every stride-2 operation
    dict(id="resnet50-f16-w2-16-A", arch="resnet50", mode="f16", world=2, N=16, V=1, hw=H.GEOMETRIES["A"], env={}, alone=True),
    # two-pass SyncBN: the parked downsample sums, bn_backward_join
    dict(id="resnet50-f32-w2-16-A", arch="resnet50", mode="f32", world=2, N=16, V=1, hw=H.GEOMETRIES["A"], env={}),
    # the mixed form of conv3_backward_linbn: bn3 by linearity, the downsample unit in two passes
    dict(id="resnet50-bf16-w2-16-C-ds0", arch="resnet50", mode="bf16", world=2, N=16, V=1, hw=H.GEOMETRIES["C"],
         env={"SM3_LINBN_DS": "0"}),
    # a by-linearity backward (both units) behind a two-pass forward
    dict(id="resnet50-bf16-w2-16-C-join0-fwd0", arch="resnet50", mode="bf16", world=2, N=16, V=1, hw=H.GEOMETRIES["C"],
         env={"SM3_LINBN_JOIN": "0", "SM3_LINBN_FWD": "0"}),
    # a world that is not 2
    dict(id="resnet50-bf16-w3-16-C", arch="resnet50", mode="bf16", world=3, N=16, V=1, hw=H.GEOMETRIES["C"], env={}),
    # the BasicBlock family
    dict(id="resnet18-bf16-w2-16-A", arch="resnet18", mode="bf16", world=2, N=16, V=1, hw=H.GEOMETRIES["A"], env={}),
    # grouped conv2: a two-pass unit beside by-linearity neighbours
    dict(id="resnext50_32x4d-bf16-w2-16-C", arch="resnext50_32x4d", mode="bf16", world=2, N=16, V=1, hw=H.GEOMETRIES["C"],
         env={}),
]
GROUPS = {w: [c for c in CASES if c["world"] == w] for w in (2, 3)}
FORM_FIELDS = ("lin", "conv3_fused", "lin_d", "join_fused", "sparse_join")


def intended_forms(case, units):
    """The form every block of the case is meant to take, from the case alone: by linearity in the 16-bit modes for a
    Bottleneck (all widths of these encoders fit the kernels' tiles), the downsample unit too unless SM3_LINBN_DS=0, the
    forward halves unless SM3_LINBN_FWD=0 (the join's also unless SM3_LINBN_JOIN=0); every stride-2 stage entry with the
    compact downsample addend (test_geometry_parity_gpu.py holds that at these geometries).  units: (has downsample, stride)."""
    on = lambda k: case["env"].get(k, "1") != "0"
    basic = case["arch"] in ("resnet18", "resnet34")
    out = []
    for has_ds, stride in units:
        sparse = has_ds and stride == 2
        lin = case["mode"] != "f32" and not basic and on("SM3_LINBN")
        lin_d = lin and has_ds and on("SM3_LINBN_DS")
        out.append((lin, lin and not has_ds and on("SM3_LINBN_FWD"), lin_d,
                    lin_d and on("SM3_LINBN_FWD") and on("SM3_LINBN_JOIN"), sparse))
    return out


def _rank_case(rank, world, case):
    import torch.distributed as dist
    torch.cuda.set_device(0)
    for k in KNOBS:  # the engine reads its switches in __init__: the case's, and nothing left over from the case before
        os.environ.pop(k, None)
    os.environ.update(case["env"])
    sync = lambda t: dist.all_reduce(t)
    dt = H.DTYPE[case["mode"]]
    h, w = case["hw"]
    run = H.engine_run(case["arch"], dt, case["N"], case["V"], h, w, DEV, rank=rank, world=world, stat_sync=sync)
    eng = run["eng"]
    assert eng.stat_sync is sync and eng.world_size == world
    name = f"{case['id']}-rank{rank}"
    rep, rest, fails = H.check_run(run, name, stat_reduce=H.all_reduce_sum)
    we, wr = H.worst(rep), H.worst(rest)
    limit = H.limits(H.bounds(case["mode"]), wr)  # the loosest limit of the case: the rule on the restatement's worst unit
    H.measure_line({"case": name + "-limit", "limit": limit})
    H.report(name, rep)
    out = dict(
        fails=[[str(f[0]), str(f[1])] + [float(v) for v in f[2:]] for f in fails], engine=we, restated=wr, limit=limit,
        forms=[tuple(bool(getattr(f, k)) for k in FORM_FIELDS) for f in run["forms"]],
        units=[(u["prefix"] + "downsample.0.weight" in run["P"], u["stride"]) for u in run["units"]],
        g_pre_relu=[bool(b) for b in run["taps"]["g_pre_relu"]], views_ran=int(run["views_ran"]),
        weights=hashlib.sha256(eng.store.flat_p.detach().cpu().numpy().tobytes()).hexdigest(), peer_effect=None)
    if case.get("alone") and rank == 0:
        # the same images through a single-rank engine (no collective: the other rank is not involved)
        xs = [t.double() for t in run["taps"]["x"]]
        del run, eng
        solo = H.engine_run(case["arch"], dt, case["N"], case["V"], h, w, DEV)
        assert solo["eng"].stat_sync is None
        out["peer_effect"] = [H.rel(a, b.double()) for a, b in zip(xs, solo["taps"]["x"])]
    return out


@pytest.fixture(scope="module")
def world2():
    return H.run_rank_group(_rank_case, 2, GROUPS[2], start_s=120, case_s=120)


@pytest.fixture(scope="module")
def world3():
    return H.run_rank_group(_rank_case, 3, GROUPS[3], start_s=120, case_s=120)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_every_unit_of_the_synchronised_step_against_fp64_by_teacher_forcing(case, request):
    from sm3hip.engine import SM3Engine
    world = case["world"]
    group = request.getfixturevalue(f"world{world}")
    res = H.group_case(group, GROUPS[world].index(case))
    if case["V"] > 1:
        assert SM3Engine.pair_ok(case["N"] // case["V"], *case["hw"])
    for r in range(world):
        o = res[r]
        print(f"\n{case['id']} rank {r}: worst over units, engine / restatement (loosest limit): "
              + ", ".join(f"{m} {o['engine'][m]:.3g} / {o['restated'][m]:.3g} ({o['limit'][m]:.3g})" for m in H.METRICS
                          if m in o["engine"]))
        assert o["views_ran"] == case["V"], o["views_ran"]
        want = intended_forms(case, o["units"])
        assert o["forms"] == want, [(i, a, b) for i, (a, b) in enumerate(zip(o["forms"], want)) if a != b]
        entries = [i for i, (_, stride) in enumerate(o["units"]) if stride == 2]
        assert len(entries) == 3 and [o["g_pre_relu"][i] for i in entries] == [True, True, True], o["g_pre_relu"]
        assert o["weights"] == res[0]["weights"], "the ranks hold different weights"
        assert not o["fails"], (r, o["fails"][:8])
    if case.get("alone"):
        effect = res[0]["peer_effect"]
        bound = H.bounds(case["mode"])["out_rel"]
        print(f"{case['id']}: rank 0's outputs against a single-rank run on the same images, per unit: "
              + ", ".join(f"{v:.2e}" for v in effect))
        assert len(effect) == len(res[0]["units"]) + 1 and min(effect) > bound, (min(effect), bound)
