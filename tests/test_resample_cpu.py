"""CPU: what the four bootstrap reports share (sm3hip/resample.py), on its own.

  * the replicate loop with a fake launch that writes a function of (seed, r0 + j): every chunk in 1 .. B gives the same arrays,
    one point call with one table, two outputs, CPU tensors;
  * safe_div: 0 and a set flag at a zero denominator, a scalar denominator broadcasts, every value has the bits of
    np.float64(a) / np.float64(b);
  * the four modules re-export the shared names as the same objects;
  * the key order of a report dict and of a comparison is the literal order the four reports had before the shared module
    (json.dump writes in that order, so the files depend on it)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = ["bootstrap", "seed", "confidence"]


def _fake_launch(calls):
    """launch(outs, seed, r0, point): table j of output i holds (seed + 1000 * (r0 + j) + 10 * i) + its flat index; -1 - i for
    the point table."""
    def launch(outs, seed, r0, point):
        calls.append((r0, outs[0].shape[0], point))
        for i, o in enumerate(outs):
            assert o.dtype == torch.int64 and not o.is_cuda
            for j in range(o.shape[0]):
                base = -1 - i if point else seed + 1000 * (r0 + j) + 10 * i
                o[j] = base + torch.arange(o[j].numel(), dtype=torch.int64).reshape(o[j].shape)
    return launch


@pytest.mark.parametrize("B", [1, 7, 12])
def test_replicate_loop_does_not_depend_on_the_chunk(B):
    from sm3hip import resample
    shapes, seed = [(2, 3), (4,)], 5
    want = [np.stack([seed + 1000 * r + 10 * i + np.arange(int(np.prod(s))).reshape(s) for r in range(B)])
            for i, s in enumerate(shapes)]
    for chunk in [None] + list(range(1, B + 1)):
        calls = []
        point, reps = resample.replicate_tables(_fake_launch(calls), shapes, B, seed, chunk, 5, torch.device("cpu"))
        c = min(B, 5) if chunk is None else chunk
        assert calls[0] == (0, 1, True) and sum(p for _, _, p in calls) == 1                 # one point call, one table
        assert calls[1:] == [(r0, min(c, B - r0), False) for r0 in range(0, B, c)]           # the short last chunk
        for i, s in enumerate(shapes):                                                       # both outputs are filled
            assert point[i].dtype == np.int64 and point[i].shape == s and reps[i].dtype == np.int64
            assert np.array_equal(point[i], -1 - i + np.arange(int(np.prod(s))).reshape(s))
            assert np.array_equal(reps[i], want[i])


def test_replicate_loop_without_a_bootstrap_is_the_point_call_alone():
    from sm3hip import resample
    calls = []
    point, reps = resample.replicate_tables(_fake_launch(calls), [(3,)], 0, 9, None, 4, torch.device("cpu"))
    assert calls == [(0, 1, True)] and reps == [None] and np.array_equal(point[0], [-1, 0, 1])


def test_safe_div_is_one_ieee_division_and_flags_a_zero_denominator():
    from sm3hip import resample
    rng = np.random.default_rng(3)
    num = rng.integers(-2 ** 40, 2 ** 40, size=(5, 7))
    den = rng.integers(1, 2 ** 40, size=(5, 7))
    den[1, 2] = den[4, 0] = 0
    v, z = resample.safe_div(num, den)
    assert v.dtype == np.float64 and z.dtype == bool and v.shape == z.shape == (5, 7)
    assert np.array_equal(z, den == 0) and v[1, 2] == 0.0 and v[4, 0] == 0.0
    for i in range(5):
        for k in range(7):
            if den[i, k]:
                assert v[i, k].tobytes() == (np.float64(num[i, k]) / np.float64(den[i, k])).tobytes()
    s, zs = resample.safe_div(num, np.int64(3) << 32)                                        # a scalar denominator broadcasts
    assert s.shape == zs.shape == (5, 7) and not zs.any()
    assert np.array_equal(s, num.astype(np.float64) / np.float64(3 << 32))
    s0, z0 = resample.safe_div(num, 0)
    assert not s0.any() and z0.all() and z0.shape == (5, 7)


def test_the_four_modules_re_export_the_shared_names():
    from sm3hip import calibration, operating, ops, report, resample, retrieval
    for name in ("interval", "interval_index", "check_settings", "MAX_BOOTSTRAP"):
        assert getattr(report, name) is getattr(resample, name)
    assert operating._div is resample.safe_div
    assert retrieval.DEFAULT_CHUNK == report.DEFAULT_CHUNK and retrieval.MAX_CASES == report.MAX_CASES
    assert retrieval.DEFAULT_CHUNK is report.DEFAULT_CHUNK and calibration.MAX_BINS is ops.CALIB_MAX_BINS


def test_interval_packing_keeps_the_key_order_of_the_four_reports():
    from sm3hip import resample
    rv, und = np.random.default_rng(1).random((6, 2, 3)), np.zeros((2, 3))
    rep = resample.pack_intervals({"values": 0, "n": 6}, [("", rv, und)], 6, 3, 0.9)         # evaluation_report
    assert list(rep) == ["values", "n", "replicates", "lo", "hi", "undefined"] + TAIL
    assert rep["undefined"].dtype == torch.int64 and rep["confidence"] == 0.9 and rep["bootstrap"] == 6 and rep["seed"] == 3
    lo, hi = resample.interval(rv, 0.9)
    assert torch.equal(rep["lo"], torch.from_numpy(lo.copy())) and torch.equal(rep["hi"], torch.from_numpy(hi.copy()))
    cal = resample.pack_intervals({}, [("label_", rv, und), ("class_", rv, und), ("diagram_", rv, und)], 6, 3, 0.9)
    assert list(cal) == [f"{t}_{k}" for t in ("label", "class", "diagram") for k in ("replicates", "lo", "hi", "undefined")] + TAIL
    ret = resample.pack_intervals({}, [("", rv, None)], 6, 3, 0.9)                           # nothing is ever undefined there
    assert list(ret) == ["replicates", "lo", "hi"] + TAIL


def test_operating_report_and_the_comparisons_keep_their_key_order():
    from sm3hip import calibration, operating, report, retrieval
    spec = importlib.util.spec_from_file_location("sm3_resample_operating_ref", os.path.join(ROOT, "tests", "test_operating_cpu.py"))
    OC = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(OC)
    preds, targets = OC.REF.make_case(9, "ties", 2)
    head = ["counts", "values", "point_undefined", "rows", "columns", "points", "thresholds", "curves", "spec_floors", "sens_floors",
            "decision", "targets", "n"]
    a = OC.host_report(preds, targets, bootstrap=3, seed=4, chunk=2)
    assert list(a) == head + ["replicates", "replicate_counts", "lo", "hi", "undefined"] + TAIL
    assert list(OC.host_report(preds, targets)) == head
    assert list(operating.compare(a, a)) == ["delta", "rows", "columns", "lo", "hi", "frac_le_zero"] + TAIL
    assert list(operating.compare(OC.host_report(preds, targets), OC.host_report(preds, targets))) == ["delta", "rows", "columns"]

    def fake(value_keys, prefixes, **more):
        rep = {k: torch.zeros(2, 3, dtype=torch.float64) for k in value_keys}
        rep.update({p + "replicates": torch.zeros(4, 2, 3, dtype=torch.float64) for p in prefixes})
        rep.update({"targets": torch.zeros(5, 8, dtype=torch.int64), "bootstrap": 4, "seed": 1, "confidence": 0.95}, **more)
        return rep
    r = fake(["values"], [""])
    assert list(report.compare(r, r)) == ["delta", "columns", "metrics", "lo", "hi", "frac_le_zero"] + TAIL
    c = fake(["label_values", "class_values"], ["label_", "class_"], n_bins=15, binning="width")
    assert list(calibration.compare(c, c)) == ["label_delta", "class_delta", "label_metrics", "label_columns", "class_metrics",
                                               "class_columns", "label_lo", "label_hi", "label_frac_le_zero", "class_lo",
                                               "class_hi", "class_frac_le_zero"] + TAIL
    t = fake(["values"], [""], N=5, ks=[1, 5], series=["R@1"], loss=0.5)
    assert list(retrieval.compare(t, t)) == ["delta", "series", "loss_delta", "lo", "hi", "frac_le_zero"] + TAIL
