"""The head of the training step against fp64, by teacher forcing (GPU).

tests/test_block_parity_gpu.py and tests/test_geometry_parity_gpu.py hold the stem and every block to fp64; their last tap
is the output of layer4.  Here everything past that tap of one SM3Trainer.step: the average pool, the in-modal projector
over 2B rows, the cross-modal projectors over B rows (one pass per pair of the style), bn7 (affine=False, fp32 output), the
NT-Xent terms with the weights 1 / 0.5 / 0.25 and the loss scale inside dz, the projector backward, the into= / addend=
accumulations of the pooled-feature gradient, the running-statistic update sequence of a projector that runs several
times per step, the metadata branch, and the pool's backward -- each recomputed in fp64 from the ENGINE'S OWN input to that
step (tests/parity_harness.py, the head section), with limit = max(BOUNDS[mode], 3 x the mode restatement's own value on
the same inputs).  The reference-only side -- the stand-in passes, every seeded defect is caught, no limit reads what the
engine returned -- is tests/test_head_parity_cpu.py.

32 x 32 images give a 1 x 1 layer4 map; the sizes are the smallest that reach each path (case 4: the benchmark's head shape).
Case 8 (kind "simclr") has no SM3Trainer -- the trainer drives the two-branch models -- so its step is forward, the
trainer's per-term NT-Xent launch and backward (parity_harness.head_step).

Measured on an MI355X (profiles/head_parity_measure.md): the engine sits on the mode restatement in every case and metric,
e.g. bf16 projections 5.3e-3 .. 6.3e-3 rel, pooled-feature gradient cosine >= 0.998 with |norm ratio - 1| 1.0e-4 .. 1.7e-3,
f16 3.1e-2 rel at most on any gradient, f32 1.4e-6; the loss within 1.2e-6 of fp64; no limit was exceeded and no defect found.

test_the_lane_schedule_changes_no_bit: the same two steps from the same state under (two_streams, lane_cross) in
{(True, True), (True, False), (False, False)} -- which stream a launch sits on is not an input of the step.
"""
import pytest
import torch

import parity_harness as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = {c["id"]: c for c in H.HEAD_CASES}
# what each case reaches
#   1  M = 128: one full row tile; cross M = 64: a partial tile
#   2  M = 144: tile + tail; four pairs; weight 0.25; three addends per feature slice; cross buffers updated four times;
#      the loss scale 1024 inside dz
#   3  swapped pairs; M = 80 / 40; another projection width
#   4  2048-wide; M = 512 / 256; both views as one batch (pair_ok: 256 rows per view on the 1 x 1 map)
#   5  one shared cross projector: interleaved statistic updates, summed parameter gradients; lane_cross forced off
#   6  exact-f32 mode; two-pass BatchNorms; BatchNorm1d over 8 / 16 rows
#   7  the metadata projector, its two extra terms, the += into dz["cross0"]
#   8  a single SimCLR branch, no lanes, a 2 x 2 map through the pool (256 rows per view: one pair batch)


@pytest.mark.parametrize("cid", list(CASES))
def test_the_head_of_the_train_step_against_fp64_by_teacher_forcing(cid):
    from sm3hip.engine import SM3Engine
    case = CASES[cid]
    run = H.head_engine_run(case, dev=DEV)
    eng = run["eng"]
    # the case ran the path it is here for
    n_pairs = len(H.cross_pairs(case["style"])) if case["kind"] != "simclr" else 0
    assert len(run["zs"]) == len(run["branches"]) + n_pairs + (1 if case["meta"] else 0)
    paired = SM3Engine.pair_ok(case["B"], case["size"], case["size"])  # both views as one batch: cases 4 (1 x 1 map) and 8
    assert paired == (cid[0] in "48") and all(run["paired"][k] == paired for k in run["branches"]), run["paired"]
    assert run["hw"] == (4 if cid.startswith("8-") else 1)
    assert run["scale"] == H.head_scale(case, run["dt"])  # no overflow step: the scale dz was made with
    if case["kind"] == "v3":
        assert eng.cross[0] is eng.cross[1] and not eng.lane_cross
    rep, rest, fails, lims = H.check_head(run, "head-" + cid)
    H.head_report("head-" + cid, rep, rest, lims)
    assert {"pool", "poolgrad", "z", "buf", "dz", "dfeat", "grad", "loss"} == set(rep)
    assert not fails, fails[:8]


LANES = [(True, True), (True, False), (False, False)]


def _state_after(case, lanes, steps):
    model, tr, eng, imgs, meta = H.head_setup(case, H.DTYPE[case["mode"]], DEV, lanes)
    losses = [H.head_step(case, tr, eng, imgs, meta) for _ in range(steps)]
    torch.cuda.synchronize()
    assert (eng.two_streams, eng.lane_cross) == lanes
    st = eng.store
    out = {"loss": torch.tensor(losses), "flat_g": st.flat_g.clone(), "flat_p": st.flat_p.clone(), "m": tr.m.clone(),
           "v": tr.v.clone()}
    out.update({"buf:" + k: b.detach().clone() for k, b in model.named_buffers()})
    return out


@pytest.mark.parametrize("cid", [c for c in CASES if c[0] in "1257"])
def test_the_lane_schedule_changes_no_bit(cid):
    """Two steps per run: the first verifies the gradient-ready schedule and runs AdamW in one launch, the second runs it
    bucket by bucket on the lane that finished the bucket (bf16; f16 keeps the single launch behind the overflow check)."""
    case = CASES[cid]
    settings = [s for s in LANES if not (case["kind"] == "v3" and s[1])]  # the shared cross projector cannot enable lane_cross
    assert len(settings) == (2 if case["kind"] == "v3" else 3)
    base = _state_after(case, settings[0], 2)
    for s in settings[1:]:
        other = _state_after(case, s, 2)
        assert set(other) == set(base)
        diff = [k for k in base if not torch.equal(base[k], other[k])]
        assert not diff, (settings[0], s, diff[:6], len(diff))
