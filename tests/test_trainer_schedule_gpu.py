"""GPU: the code that decides WHEN and OVER WHICH SLICE the optimizer kernels run -- SM3Trainer._step and the gradient-ready
notifications of SM3Engine.backward -- under every AdamW schedule the trainer has:

  1. the "verify" step (first step of a configuration: notifications recorded, one launch at the end),
  2. the early path (AdamW bucket by bucket from inside backward, on the lane that finished the bucket),
  3. SM3_ADAMW_BUCKETS=0 (one launch after backward, every step),
  4. data parallel (AdamW per bucket behind that bucket's all-reduce, grad_scale 1 / world),
  5. a loss scale (fp16: check_finite -> adamw_dynamic -> loss_scale_update, the step counted on the device),

each followed by the optional momentum target.  Gradients are a function of their inputs, AdamW is a per-element function
whose bits do not depend on the launch, so every schedule must give the SAME BITS, and each step can be replayed from its
own before / after state (schedule_inputs.checked_step: one sm3_adamw launch, the fp64 oracle inside edge_inputs' bounds,
one sm3_ema_update launch, the filter banks against the masters the last forward read).

A difference here is a bug in trainer.py / engine.py, not a tolerance: first_diff() names the first differing parameter,
which maps to a bucket, a stream and a step."""
import os
import socket
import sys
import traceback

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import schedule_inputs as S
from schedule_inputs import DEV, ROWS, checked_step

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 4
VARIANTS = ("default", "one_launch", "one_stream", "cross_on_main")


def _start(row, variant):
    model = S.row_model(row)
    tr = S.row_trainer(row, model)
    eng = tr._engine()
    assert eng.det_wgrad
    if variant == "one_stream":
        eng.two_streams = False
    if variant == "cross_on_main":
        assert eng.cross[0] is not eng.cross[1] and eng.lane_cross
        eng.lane_cross = False
    return model, tr, eng


def _run(row, variant, steps=STEPS, against=None):
    """`steps` checked steps of one schedule from the row's initial state; compared step by step with the records
    `against` (of another schedule) when given."""
    model, tr, eng = _start(row, variant)
    B, (H, W) = ROWS[row][3], ROWS[row][4]
    if B == 32:
        assert eng.pair_ok(B, H, W)  # both views of a branch as one batch
    recs = []
    for i, batch in enumerate(S.row_batches(row, steps)):
        rec = checked_step(tr, batch, tag=f"{row} {variant} step {i + 1}")
        # the schedule that was meant is the one that ran: only a verified configuration takes the early path
        assert (tr.__dict__.get("_sched_ok") is not None) == (variant != "one_launch"), (row, variant)
        assert tr.step_count == i + 1
        if against is not None:
            S.assert_same_step(against[i], rec, eng.store, f"{row}: default vs {variant}, step {i + 1}")
        recs.append(rec if against is None else None)
    return recs, eng.store


_default_runs = {}


def _default_run(row):
    """The uninterrupted default schedule (verify step, then early buckets) of a row, kept for the rows that the resume
    test compares with."""
    if row not in _default_runs:
        recs, store = _run(row, "default")
        for a, b in zip(recs, recs[1:]):  # not vacuous: every step moves the bits
            assert not torch.equal(a["loss"], b["loss"])
            assert not any(S.same_bits(a[k], b[k]) for k in ("p", "m", "v", "g"))
            assert any(not S.same_bits(x, b["buffers"][k]) for k, x in a["buffers"].items())
            if a["target"] is not None:
                assert not S.same_bits(a["target"], b["target"])
        if row not in RESUME_ROWS:
            return recs, store
        _default_runs[row] = (recs, store)
    return _default_runs[row]


RESUME_ROWS = (list(ROWS)[0], list(ROWS)[-1])


@pytest.mark.parametrize("row", list(ROWS))
def test_every_single_rank_schedule_gives_the_same_bits(row, monkeypatch):
    """Four steps on four batches from one state under (a) the default schedule, (b) SM3_ADAMW_BUCKETS=0, (c) one stream,
    (d) the cross projectors on the main stream: loss, parameters, moments, gradients, running statistics and the target
    are equal bit for bit after every step, and every step of every schedule passes its own replay."""
    monkeypatch.delenv("SM3_ADAMW_BUCKETS", raising=False)
    ref, _store = _default_run(row)
    for variant in VARIANTS[1:]:
        if variant == "cross_on_main" and ROWS[row][0] == "v3":
            continue  # one shared cross projector: it runs on the main stream after the join as it is
        if variant == "one_launch":
            monkeypatch.setenv("SM3_ADAMW_BUCKETS", "0")
        else:
            monkeypatch.delenv("SM3_ADAMW_BUCKETS", raising=False)
        _run(row, variant, against=ref)


@pytest.mark.parametrize("row", RESUME_ROWS)
def test_resume_after_step_two_continues_bit_for_bit(row, monkeypatch):
    """state_dict / optimizer_state_dict / scaler_state_dict after step 2 -> a fresh model and a fresh trainer -> steps 3
    and 4.  The fresh trainer's first step is a verify step where the uninterrupted run takes a bucketed one; both steps
    still equal the uninterrupted run bit for bit."""
    monkeypatch.delenv("SM3_ADAMW_BUCKETS", raising=False)
    ref, _store = _default_run(row)
    batches = S.row_batches(row, STEPS)
    model, tr, eng = _start(row, "default")
    for i in range(2):
        S.assert_same_step(ref[i], checked_step(tr, batches[i], tag=f"{row} before the checkpoint, step {i + 1}"),
                           eng.store, f"{row}: step {i + 1}")
    ck = {"state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
          "optimizer": tr.optimizer_state_dict(), "scaler": tr.scaler_state_dict()}
    # the checkpoint format has no place for the momentum target: it is handed over directly
    target = tr.flat_target.clone() if tr.flat_target is not None else None
    del model, tr, eng

    fresh = S.row_model(row)
    assert not fresh.load_state_dict(ck["state_dict"], strict=True).missing_keys
    tr2 = S.row_trainer(row, fresh)
    tr2.lr = 123.0  # every hyper-parameter comes from the checkpoint
    tr2.load_optimizer_state_dict(ck["optimizer"])
    tr2.load_scaler_state_dict(ck["scaler"])
    tr2.flat_target = target
    eng2 = tr2._engine()
    assert tr2.step_count == 2 and tr2.__dict__.get("_sched_ok") is None
    assert S.same_bits(eng2.store.flat_p, ref[1]["p"]) and S.same_bits(tr2.m, ref[1]["m"]) and S.same_bits(tr2.v, ref[1]["v"])
    for i in (2, 3):
        rec = checked_step(tr2, batches[i], tag=f"{row} resumed, step {i + 1}")
        S.assert_same_step(ref[i], rec, eng2.store, f"{row}: resumed step {i + 1}")
    assert tr2.__dict__.get("_sched_ok") is not None
    _default_runs.pop(row, None)  # the last user of the row's records: give the memory back


# ---- the loss-scale path (fp16) ------------------------------------------------------------------------------------------
OVERFLOW_SCALE = 65536.0  # the scale test_fp16_gradscaler_backoff_sequence_b4 overflows from (the trainer's default)


def _fp16_model():
    return S.fresh_model("v32", "resnet18", torch.float16)


def test_fp16_loss_scale_steps_replay():
    """check_finite -> adamw_dynamic -> loss_scale_update: three clean steps, each equal to one sm3_adamw launch with
    grad_scale 1 / scale (exact: the scale is a power of two) and the step index the device counted."""
    tr = S.make_trainer(_fp16_model(), init_scale=256.0)
    recs = [checked_step(tr, b, tag=f"fp16 step {i + 1}") for i, b in enumerate(S.make_batches(4, (64, 64), 3))]
    assert tr.steps_taken() == 3 and float(tr._scaler["scale"]) == 256.0
    assert not S.same_bits(recs[0]["p"], recs[1]["p"]) and not S.same_bits(recs[1]["p"], recs[2]["p"])


@pytest.mark.parametrize("target", [None, 0.9], ids=["plain", "momentum_target"])
def test_fp16_overflow_skips_the_step_and_leaves_the_target(target):
    """A step whose scaled gradients overflow: parameters and moments unchanged bit for bit, the scale halved, no step
    counted -- and the momentum target unchanged too ("a skipped step must not move the target either", trainer.py).
    The target differs from the online network when the overflow comes (one clean step first), or nothing could pull it."""
    model = _fp16_model()
    batches = S.make_batches(4, (64, 64), 2)
    tr = S.make_trainer(model, init_scale=256.0, target_momentum=target)
    checked_step(tr, batches[0], tag="fp16 clean step")
    eng = tr._engine()
    if target is not None:
        assert not S.same_bits(tr.flat_target, eng.store.flat_p)
    big = S.make_trainer(model, init_scale=OVERFLOW_SCALE, target_momentum=target)
    big.load_optimizer_state_dict(tr.optimizer_state_dict())
    big.flat_target = tr.flat_target  # (no place in the checkpoint format: handed over directly)
    assert big._engine() is eng and big.step_count == 1
    before = [t.clone() for t in (eng.store.flat_p, big.m, big.v)] + ([big.flat_target.clone()] if target is not None else [])
    derm, clinic, _ = batches[1]
    big.step(derm, clinic)
    torch.cuda.synchronize()
    assert float(big._scaler["scale"]) == 0.5 * OVERFLOW_SCALE, "the scaled gradients did not overflow"
    assert big.steps_taken() == 1 and int(big._scaler["found_inf"]) == 0
    after = [eng.store.flat_p, big.m, big.v] + ([big.flat_target] if target is not None else [])
    for name, a, b in zip(("p", "exp_avg", "exp_avg_sq", "target"), before, after):
        assert S.same_bits(a, b), (name, S.first_diff(eng.store, a, b))


# ---- data parallel: two ranks on the one GPU over gloo, started as tests/test_dp_gpu.py starts them ----------------------
def _rank_main(rank, world, port, q, buckets, out_dir):
    try:
        if not buckets:
            os.environ["SM3_ADAMW_BUCKETS"] = "0"
        else:
            os.environ.pop("SM3_ADAMW_BUCKETS", None)
        for p in (ROOT, os.path.join(ROOT, "skin-sm3_amd"), os.path.join(ROOT, "tests")):
            if p not in sys.path:
                sys.path.insert(0, p)
        torch.set_num_threads(6)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        import schedule_inputs as S
        Bl, steps = 4, 3
        model = S.fresh_model("v32", "resnet18", torch.float32)
        model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model).to(S.DEV)
        tr = S.make_trainer(model)
        assert tr.dp and tr.sync_bn and tr.world == world
        # The schedule that was meant is the one that ran: `dp_buckets` is a local of _step, and a schedule that does not
        # tile falls back to one launch in silence -- which replays just as well.  So the trainer's own sm3_adamw launches
        # are recorded: (offset in flat_p, length, grad_scale) of every launch whose p lies inside the flat buffer (the
        # replay of checked_step works on a clone and is not among them).
        from sm3hip import ops
        launches, real_adamw = [], ops.adamw

        def recording_adamw(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale=1.0, found_inf=None):
            flat = tr._engine().store.flat_p
            off = (p.data_ptr() - flat.data_ptr()) // 4
            if 0 <= off < flat.numel():
                launches.append((off, p.numel(), grad_scale))
            return real_adamw(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, found_inf)

        ops.adamw = recording_adamw
        sl = slice(rank * Bl, (rank + 1) * Bl)
        out = []
        for i, (derm, clinic, _) in enumerate(S.make_batches(Bl * world, (64, 64), steps)):
            del launches[:]
            rec = S.checked_step(tr, ([t[sl].contiguous() for t in derm], [t[sl].contiguous() for t in clinic], None),
                                 tag=f"rank {rank} step {i + 1}")  # flat_g: the all-reduced SUM, applied with 1 / world
            assert tr.step_count == i + 1
            total = tr._engine().store.total
            if buckets:  # AdamW behind every bucket's all-reduce: several launches that tile [0, total) exactly once
                assert len(launches) > 1, launches
                pos = 0
                for off, n, _gs in sorted(launches):
                    assert off == pos and n > 0, (launches, pos)
                    pos += n
                assert pos == total, (pos, total)
            else:
                assert [(off, n) for off, n, _gs in launches] == [(0, total)], launches
            out.append({k: rec[k].cpu() for k in ("p", "m", "v")} | {"loss": float(rec["loss"].view(torch.float32))})
        # (the tensors go through a file: 3 steps x 3 buffers of 25 M floats are too much for a queue's shared memory)
        path = os.path.join(out_dir, f"rank{rank}.pt")
        torch.save(out, path)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, True, path))
    except Exception:
        q.put((rank, False, traceback.format_exc()))


_dp_bucketed = {}


def _dp_run(buckets, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, q, buckets, out_dir)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(2):
            r, ok, payload = q.get(timeout=300)
            assert ok, f"rank {r} failed:\n{payload}"
            res[r] = torch.load(payload, map_location="cpu")
        for p in procs:
            p.join(timeout=60)
    finally:  # a rank that failed leaves its peer inside a collective: do not let it hold the GPU until gloo times out
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    for i, (a, b) in enumerate(zip(res[0], res[1])):
        assert a["loss"] != b["loss"]  # different shards
        for k in ("p", "m", "v"):
            assert S.same_bits(a[k], b[k]), (f"replicas differ after step {i + 1}", k, int((a[k] != b[k]).sum()))
    assert not S.same_bits(res[0][0]["p"], res[0][1]["p"]) and not S.same_bits(res[0][1]["p"], res[0][2]["p"])
    return res[0]


@pytest.mark.parametrize("buckets", [True, False], ids=["per_bucket", "one_launch"])
def test_two_rank_dp_steps_replay_and_replicas_stay_equal(buckets, tmp_path):
    """Three data-parallel steps (resnet18, 4 pairs per rank, f32): every step of every rank passes its replay with
    grad_scale 1 / world on the all-reduced gradient, the replicas hold the same bits after every step, and AdamW behind
    every bucket's all-reduce gives the bits of SM3_ADAMW_BUCKETS=0 (one launch behind the last)."""
    if "run" not in _dp_bucketed:
        _dp_bucketed["run"] = _dp_run(True, str(tmp_path / "per_bucket"))
    if buckets:
        return
    one = _dp_run(False, str(tmp_path / "one_launch"))
    for i, (a, b) in enumerate(zip(_dp_bucketed["run"], one)):
        assert a["loss"] == b["loss"], i
        for k in ("p", "m", "v"):
            assert S.same_bits(a[k], b[k]), (f"per bucket vs one launch, step {i + 1}", k, int((a[k] != b[k]).sum()))
