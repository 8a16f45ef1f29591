"""The head section of tests/parity_harness.py on the reference alone -- no GPU, nothing of the library.

  * the harness's own restatements of reference code are held to that code: proj_ref with no stores is
    oracle.sm3_oracle.projector bit for bit, cross_pairs is the pair table sm3_v32_projections applies, cross_weight the
    weight sm3_loss applies;
  * the stand-in (head_standin_run: the mode restatement of the head chained from synthetic layer4 maps) passes check_head
    for the eight configurations of tests/test_head_parity_gpu.py in bf16, f16 and f32;
  * the rule does not turn vacuous: in every 16-bit case the limit applied to the norm ratio of a pooled-feature gradient
    stays <= 3e-3 and the limit applied to a cosine >= 0.97;
  * every seeded defect, alone, puts the tensor named in its assertion over its limit;
  * no limit depends on what the run returned for the step it bounds (head_limits on poisoned outputs).
"""
import copy

import pytest
import torch

import parity_harness as H

MODES = ["bf16", "f16", "f32"]
CASES = {c["id"].split("-")[0]: c for c in H.HEAD_CASES}


def test_proj_ref_without_stores_is_the_oracles_projector():
    from oracle import sm3_oracle as O
    run = H.head_standin_run(CASES["3"], torch.float32)
    P = {n: w.double() for n, w in run["P"].items()}
    x = run["ft"]["derm"].double()
    B1 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in run["buf0"].items()}
    B2 = copy.deepcopy(B1)
    a = H.proj_ref(x, P, B1, "cross_proj.0.")
    b = O.projector(x, P, B2, "cross_proj.0.", True)
    assert torch.equal(a, b) and all(torch.equal(B1[k], B2[k]) for k in B1)
    assert int(B1["cross_proj.0.7.num_batches_tracked"]) == 1


@pytest.mark.parametrize("style", [0, 1, 2])
def test_pair_table_and_cross_weight_are_the_oracles(style, monkeypatch):
    from oracle import sm3_oracle as O
    # sm3_v32_projections with the encoder replaced by view markers and the projector by the identity: its cross outputs
    # then spell the pair table
    mark = {"derm_backbone.": (torch.tensor([[10.0]]), torch.tensor([[11.0]])),
            "clinic_backbone.": (torch.tensor([[20.0]]), torch.tensor([[21.0]]))}
    monkeypatch.setattr(O, "simclr_projections", lambda x1, x2, P, B, prefix, *a: (torch.zeros(2, 1), mark[prefix]))
    monkeypatch.setattr(O, "projector", lambda x, *a: x)
    zs = O.sm3_v32_projections({}, {}, [None, None], [None, None], style)
    got = [(int(z[0]) - 10, int(z[1]) - 20) for z in zs[2:]]
    assert got == H.cross_pairs(style)
    monkeypatch.undo()
    g = torch.Generator().manual_seed(style)
    lg = [torch.randn(6, 5, generator=g, dtype=torch.float64) for _ in range(2 + len(got))]
    outs = ((lg[0], None), (lg[1], None), tuple((t, None) for t in lg[2:]))
    ce = O.cross_entropy_zero_label
    want = ce(lg[0]) + ce(lg[1]) + sum(H.cross_weight(style) * ce(t) for t in lg[2:])
    assert abs(float(O.sm3_loss(outs, style)) - float(want)) < 1e-14


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cid", list(CASES))
def test_the_stand_in_passes_and_the_rule_is_not_vacuous(cid, mode):
    case, dt = CASES[cid], H.DTYPE[mode]
    run = H.head_standin_run(case, dt)
    rep, rest, fails, lims = H.check_head(run, f"cpu-head-{cid}-{mode}")
    H.head_report(f"cpu-head-{cid}-{mode}", rep, rest, lims)
    assert not fails, fails[:8]
    # every class of tensor was compared, every buffer of every projector
    stages = {"pool", "poolgrad", "z", "buf", "dz", "dfeat", "grad", "loss"}
    assert set(rep) == stages, set(rep) ^ stages
    assert len([n for n in lims if n.startswith("buf:")]) == 6 * len({c["prefix"] for c in run["calls"]})
    if mode != "f32":
        for name, lim in lims.items():
            assert lim.get("in_ratio", 0.0) <= 3e-3 and lim.get("cos", 1.0) >= 0.97, (name, lim)


def _names(fails):
    return [f[0] for f in fails]


# defect -> (case, mode, the tensor that must leave its limit)
DEFECTS = {
    "pairs_style0": ("3", "bf16", "z:cross0"),
    "cross_weight_half": ("2", "f16", "dz:cross1"),
    "cross_bn_2B": ("1", "bf16", "z:cross0"),
    "cross_stats_once": ("2", "f16", "buf:cross_proj.1.4.running_mean"),
    "v3_order": ("5", "f16", "buf:cross_proj.1.running_mean"),
    "bn7_affine": ("1", "bf16", "z:derm"),
    "drop_into": ("2", "f16", "dfeat:derm"),
    "addend_view0": ("1", "bf16", "dfeat:clinic"),
    "dz_scaled": ("2", "f16", "dz:derm"),
    "meta_not_added": ("7", "bf16", "dz:cross0"),
    "pool_twice": ("8", "bf16", "poolgrad:main"),
}


def test_every_defect_of_the_harness_is_seeded_here():
    assert set(DEFECTS) == set(H.HEAD_DEFECTS)


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_a_seeded_defect_leaves_its_limit(defect):
    cid, mode, tensor = DEFECTS[defect]
    run = H.head_standin_run(CASES[cid], H.DTYPE[mode], defects=(defect,))
    _, _, fails, _ = H.check_head(run, f"cpu-head-{cid}-{mode}-{defect}")
    print(f"\n{defect}:", [f for f in fails if f[0] == tensor][:2], "... of", len(fails))
    assert tensor in _names(fails), (defect, tensor, _names(fails)[:12])


def test_a_second_step_of_the_cross_statistics_is_counted():
    """cross_stats_once also shows in num_batches_tracked, which is held exactly."""
    run = H.head_standin_run(CASES["2"], torch.float16, defects=("cross_stats_once",))
    _, _, fails, _ = H.check_head(run, "cpu-head-2-f16-count")
    assert "buf:cross_proj.0.1.num_batches_tracked" in _names(fails)
    assert H.nbt_expected(run)["cross_proj.0.1.num_batches_tracked"] == 4
    v3 = H.head_standin_run(CASES["5"], torch.float32)
    assert H.nbt_expected(v3)["cross_proj.7.num_batches_tracked"] == 8
    assert H.nbt_expected(v3)["derm_backbone.projector.1.num_batches_tracked"] == 1


def test_no_limit_depends_on_what_the_run_returned_for_that_step():
    """head_limits on a run whose outputs are poisoned: the tensors only ever compared (fp32 features, tap gradients, buffers,
    parameter gradients, the loss) move no limit at all; a tensor that is the output of one step and the input of the next
    moves no limit of the step that produced it."""
    run = H.head_standin_run(CASES["7"], torch.bfloat16)
    _, vals, lims = H.head_limits(run)
    nan = lambda t: torch.full_like(t, float("nan")) if t.is_floating_point() else t + 7
    bad = dict(run)
    for k in ("f32", "tap_g", "bufs", "grads"):
        bad[k] = {n: nan(t) for n, t in run[k].items()}
    bad["loss"] = float("nan")
    _, vals2, lims2 = H.head_limits(bad)
    assert lims2 == lims and vals2 == vals
    produced_by = {"ft": "pool:", "zs": "z:", "dz": "dz:", "dfeat": "dfeat:"}
    for k, stage in produced_by.items():
        bad = dict(run)
        bad[k] = {n: t * 1.5 for n, t in run[k].items()}
        _, _, lims2 = H.head_limits(bad)
        mine = [n for n in lims if n.startswith(stage)]
        assert mine and all(lims2[n] == lims[n] for n in mine), (k, stage)
