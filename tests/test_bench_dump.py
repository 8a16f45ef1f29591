"""bench.py --dump-outputs DIR: after the timed steps, what the last timed step handed its caller is written as DIR/<name>.npy
(float32, 64 MB at most), from inputs that are the same on every run with the same arguments -- so that two builds can be
compared output for output.  On CPU through the dry-run mode (kernels stubbed by tests/fakelib.py: the file contract and its
fixed sample), on the GPU through the real timed path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRETRAIN_OUTPUTS = {"loss.npy", "params.npy", "grads.npy", "bn_buffers.npy"}
BUDGET = 64 << 20


def _bench(out_dir, *extra, env_extra=None, timeout=600):
    env = dict(os.environ, **(env_extra or {}))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", str(out_dir), *extra],
                        env=env, capture_output=True, text=True, timeout=timeout)
    assert pr.returncode == 0, pr.stderr[-3000:]
    lines = [json.loads(l) for l in pr.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, pr.stdout
    return lines[0], {f: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}


def _check_files(arrays):
    assert set(arrays) == PRETRAIN_OUTPUTS
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= BUDGET
    assert arrays["loss.npy"].shape == (1,)
    # 81.6 M parameters: parameters and gradients are the same seeded sample of them
    assert arrays["params.npy"].shape == arrays["grads.npy"].shape and 4_000_000 < arrays["params.npy"].size <= 1 << 22


def test_dry_run_dump_is_the_same_fixed_sample_every_run(tmp_path):
    recs, dumps = [], []
    for run in ("a", "b"):
        rec, arrays = _bench(tmp_path / run, "--steps", "1", "--warmup", "0", env_extra={"SM3_BENCH_DRYRUN": "1"}, timeout=300)
        _check_files(arrays)
        recs.append(rec)
        dumps.append(arrays)
    assert recs[0]["dry_run"] is True
    for name in PRETRAIN_OUTPUTS:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name
    assert np.abs(dumps[0]["params.npy"]).sum() > 0  # the seeded initial weights (no kernel ran to move them)


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step_and_repeats_it(tmp_path):
    """Two runs with the same arguments: the files hold the loss the JSON line reports, finite parameters, gradients and
    BatchNorm buffers of the last timed step, and the second run lands on the first within the run-to-run spread of the
    float-atomic weight gradients."""
    args = ("--steps", "3", "--warmup", "1", "--batch", "32", "--img", "64", "--no-cpu-baseline", "--no-other-dtypes")
    (ra, a), (rb, b) = (_bench(tmp_path / run, *args) for run in ("a", "b"))
    for rec, arrays in ((ra, a), (rb, b)):
        _check_files(arrays)
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0
        assert abs(float(arrays["loss.npy"][0]) - rec["config"]["loss"]) <= 1e-5
        assert all(np.isfinite(x).all() for x in arrays.values())
        assert np.abs(arrays["grads.npy"]).max() > 0
    g_a, g_b = a["grads.npy"].astype(np.float64), b["grads.npy"].astype(np.float64)
    cos = float(g_a @ g_b / (np.linalg.norm(g_a) * np.linalg.norm(g_b)))
    loss_rel = abs(float(a["loss.npy"][0]) - float(b["loss.npy"][0])) / abs(float(a["loss.npy"][0]))
    param_diff = float(np.abs(a["params.npy"] - b["params.npy"]).max())
    buf_diff = float(np.abs(a["bn_buffers.npy"] - b["bn_buffers.npy"]).max())
    print(f"run to run: loss rel {loss_rel:.2e}, gradient cosine {cos:.8f}, params max {param_diff:.2e}, "
          f"BN buffers max {buf_diff:.2e}")
    assert loss_rel <= 1e-2 and cos >= 0.99 and param_diff <= 1e-5
