"""CPU: the significance tests of a paired comparison (sm3hip/significance.py, csrc/signif.hip) -- everything that needs no GPU.
tests/signif_inputs.py holds the cases and the by-definition restatements.

  * DeLong: the worked example of the module's contract to the bits; the module's host arithmetic == the Fraction restatement
    on tied inputs; the exact variance against the float definition (np.cov of the V10 / V01 components) within a bound derived
    from the lengths of the sums;
  * the kernel's route (one joint ranking, tie groups, per-side prefix sums) in numpy == the counts of swapped predictions that
    are formed and recounted, N = 1 .. 257, and the unswapped record == the evaluation report's integer restatement;
  * the swap stream: the module's bits == the restatement's; every case of N = 200 is swapped in 40 % to 60 % of 2048 replicates;
  * Holm and McNemar against scipy.stats.binomtest, the restatement and hand cases;
  * every refusal, in order: unequal targets, N over the limit, NaN, bad permutations / seed / chunk, --significance without
    --against;
  * ABI 9 with the two symbols in the header, the binding and the built library, and their -1 / -2 before any launch."""
import ctypes as C
import importlib.util
import math
import os
import statistics
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "skin-sm3_amd", "tools")


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, file)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SI = _load("sm3_signif_inputs", os.path.join(ROOT, "tests", "signif_inputs.py"))
U = 2.0 ** -53


# ---- 1. DeLong --------------------------------------------------------------------------------------------------------------
def test_worked_example_to_the_bits():
    from sm3hip import significance
    pos = np.array([1, 1, 1, 0, 0, 0, 0], dtype=bool)
    a = np.array([.9, .4, .6, .5, .3, .1, .4])
    b = np.array([.8, .6, .2, .7, .2, .1, .3])
    pa, pb = SI.placements_by_psi(a, pos), SI.placements_by_psi(b, pos)
    assert pa.tolist() == [8, 5, 8, 4, 6, 6, 5]                                       # case 1 ties with case 6: 2 * 2 + 1
    ta, tb, var, _, _ = SI.delong_exact(pa[pos], pb[pos], pa[~pos], pb[~pos])
    assert (ta, tb, var) == (Fraction(7, 8), Fraction(17, 24), Fraction(101, 1728))
    one = significance.delong_column(pa[pos], pb[pos], pa[~pos], pb[~pos])
    assert one["theta_a"] == 7 / 8 and one["theta_b"] == 17 / 24 and one["var"] == 101 / 1728
    assert one["z"] == 0.6893819875457112 and one["p"] == 0.4905829155605297 and not one["undefined"]
    assert one["delta"] == float(Fraction(1, 6)) and one["lo"] < 0 < one["hi"]
    zc = statistics.NormalDist().inv_cdf(0.975)
    assert abs(zc - 1.959964) < 1e-6 and one["lo"] == one["delta"] - zc * math.sqrt(101 / 1728)


@pytest.mark.parametrize("kind", ["other", "permuted", "same", "sparse"])
def test_module_delong_equals_the_fraction_restatement(kind):
    from sm3hip import significance
    a, b, targets = SI.make_pair(61, kind, 3)
    sa, sb, y = SI.scores(a), SI.scores(b), targets.numpy()
    pa = np.stack([SI.placements_by_psi(sa[k], y[:, t] == c) for k, (t, c) in enumerate(SI.PAIRS)])
    pb = np.stack([SI.placements_by_psi(sb[k], y[:, t] == c) for k, (t, c) in enumerate(SI.PAIRS)])
    got = significance.delong_from_placements(pa, pb, y, 0.9)
    seen = set()
    for k, (t, c) in enumerate(SI.PAIRS):
        pos = y[:, t] == c
        ta, tb, var, va, vb = SI.delong_exact(pa[k][pos], pb[k][pos], pa[k][~pos], pb[k][~pos])
        z, p, undefined = SI.delong_z_p(ta, tb, var)
        assert (float(got["z"][k]), float(got["p"][k]), bool(got["undefined"][k])) == (z, p, undefined), k
        assert float(got["theta_a"][k]) == float(ta) and float(got["theta_b"][k]) == float(tb)
        assert float(got["var"][k]) == (0.0 if var is None else float(var))
        assert float(got["var_a"][k]) == (0.0 if va is None else float(va))
        seen.add(undefined)
        # sum of the doubled placements of the positives = the report's A2
        assert int(pa[k][pos].sum()) == SI.a2_by_definition(sa[k], pos)
    assert seen == ({True} if kind == "same" else {True, False} if kind in ("sparse", "permuted") else {False})
    assert np.array_equal(got["p_holm_classes"].numpy(), SI.holm_by_definition(got["p"].numpy()))
    sel = [SI.PAIRS.index((t, w)) for t, w in enumerate(significance.report.CLS_WEIGHTS)]
    assert sel == significance.SELECTED
    assert np.array_equal(got["p_holm_selected"].numpy(), SI.holm_by_definition(got["p"].numpy()[sel]))


def test_exact_variance_against_the_float_definition():
    """The float definition: S10 = np.cov of the components V10_x = u^x / (2 Q) over the P positives, S01 = np.cov of V01_x = v^x /
    (2 P) over the Q negatives, S = S10 / P + S01 / Q, Var = S_aa + S_bb - 2 S_ab.  The exact rational is the yardstick.

    Bound, for one covariance entry of n components in [0, 1] (u = 2^-53): the mean is a sum of n terms and a division, so each
    deviation carries an absolute error of at most eta = (n + 2) u; the sum of the n products of deviations then errs by at most
    2 eta sqrt(n) sqrt((n - 1) s) + n eta^2 from the deviations (Cauchy-Schwarz, s = the larger of the two variances) and by
    (n + 2) u of the sum of the absolute products <= (n - 1) sqrt(s_x s_y) from its own roundings; all divided by n - 1.  With
    scale = S_aa + S_bb + 2 |S_ab| >= each s, the four entries of Var (aa, bb, twice ab) err by at most
        4 * (2 eta sqrt(n / (n - 1)) sqrt(scale) + n eta^2 / (n - 1)) + (n + 2) u scale
    per component matrix; the divisions by P and Q and the three last additions add 6 u of the total scale."""
    worst = 0.0
    for N, kind, seed in ((61, "other", 3), (257, "other", 5), (257, "permuted", 7), (1000, "other", 9)):
        a, b, targets = SI.make_pair(N, kind, seed)
        sa, sb, y = SI.scores(a), SI.scores(b), targets.numpy()
        for k, (t, c) in enumerate(SI.PAIRS):
            pos = y[:, t] == c
            P, Q = int(pos.sum()), int((~pos).sum())
            pa, pb = SI.placements_by_psi(sa[k], pos), SI.placements_by_psi(sb[k], pos)
            _, _, var, _, _ = SI.delong_exact(pa[pos], pb[pos], pa[~pos], pb[~pos])
            s10 = np.cov(np.stack([pa[pos] / (2.0 * Q), pb[pos] / (2.0 * Q)]))
            s01 = np.cov(np.stack([pa[~pos] / (2.0 * P), pb[~pos] / (2.0 * P)]))
            S = s10 / P + s01 / Q
            got = S[0, 0] + S[1, 1] - 2.0 * S[0, 1]
            bound = 0.0
            for n, m in ((P, s10), (Q, s01)):
                eta, scale = (n + 2) * U, m[0, 0] + m[1, 1] + 2.0 * abs(m[0, 1])
                bound += (4.0 * (2.0 * eta * math.sqrt(n / (n - 1.0)) * math.sqrt(scale) + n * eta * eta / (n - 1.0))
                          + (n + 2) * U * scale) / n
            total = S[0, 0] + S[1, 1] + 2.0 * abs(S[0, 1])
            bound += 6.0 * U * total
            err = abs(got - float(var))
            worst = max(worst, err / bound if bound else 0.0)
            assert err <= bound, (N, kind, k, got, float(var), bound)
    print(f"largest |float - exact| / bound: {worst:.3g}")


# ---- 2. the kernel's route, in numpy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 31, 32, 33, 129, 257])
def test_joint_ranking_counts_equal_the_recount_of_swapped_predictions(N):
    ref = SI.report_ref()
    for kind in ("other", "permuted", "same", "sparse"):
        a, b, targets = SI.make_pair(N, kind, 11 * N)
        sa, sb, ha, hb, y = SI.scores(a), SI.scores(b), SI.argmax(a), SI.argmax(b), targets.numpy()
        none = np.zeros(N, dtype=bool)
        point = SI.joint_counts(sa, sb, ha, hb, y, none)
        assert np.array_equal(point, SI.recount(sa, sb, ha, hb, y, none)), kind
        full = SI.full_counts(point, y)
        for w, preds in enumerate((a, b)):                                           # the report's own integer restatement
            assert np.array_equal(full[w], ref.counts(*ref.restated_inputs(preds, targets), np.ones(N, dtype=np.int64))), (kind, w)
        for r in (0, 1, 2):
            swap = SI.swap_bits(2 ** 63 + 11, r, N)
            assert np.array_equal(SI.joint_counts(sa, sb, ha, hb, y, swap), SI.recount(sa, sb, ha, hb, y, swap)), (kind, r)


def test_full_counts_of_the_module():
    from sm3hip import significance
    a, b, targets = SI.make_pair(33, "other", 1)
    y = targets.numpy()
    side = SI.recount(SI.scores(a), SI.scores(b), SI.argmax(a), SI.argmax(b), y, SI.swap_bits(0, 0, 33))
    assert np.array_equal(significance.full_counts(side, y), SI.full_counts(side, y))
    assert np.array_equal(significance.full_counts(np.stack([side, side]), y)[1], SI.full_counts(side, y))


# ---- 3. the swap stream ------------------------------------------------------------------------------------------------------
def test_swap_bits_are_the_restatement_and_a_fair_coin():
    from sm3hip import resample, significance
    for seed, r, N in ((0, 0, 1), (7, 3, 31), (2 ** 32 + 5, 1000, 33), (2 ** 63 + 11, 2 ** 20, 129), (1, 2, 513), (9, 4, 8192)):
        got = significance.swap_bits(seed, r, N)
        assert got.dtype == bool and got.shape == (N,) and np.array_equal(got, SI.swap_bits(seed, r, N)), (seed, r, N)
    assert not np.array_equal(significance.swap_bits(7, 3, 513), significance.swap_bits(7, 4, 513))
    assert not np.array_equal(significance.swap_bits(7, 3, 513), significance.swap_bits(2 ** 32 + 7, 3, 513))  # the high key word
    assert np.array_equal(significance.swap_bits(7, 3, 513)[:200], significance.swap_bits(7, 3, 200))     # a function of i, not of N
    # stream 5 is apart from the bootstrap's 2
    assert significance.STREAM == 5 and not np.array_equal(resample.philox_words(8, 1, 0, 5), resample.philox_words(8, 1, 0, 2))
    share = np.mean([significance.swap_bits(0, r, 200) for r in range(2048)], axis=0)
    print(f"swapped in {100 * share.min():.1f} % to {100 * share.max():.1f} % of 2048 replicates")
    assert share.min() >= 0.40 and share.max() <= 0.60


# ---- 4. Holm, McNemar ----------------------------------------------------------------------------------------------------
def test_holm():
    from sm3hip import significance
    got = significance.holm([0.01, 0.04, 0.03, 0.005])
    assert got.tolist() == [3 * 0.01, 2 * 0.03, 2 * 0.03, 4 * 0.005]                   # 0.04 * 1 stays under the running maximum
    assert significance.holm([0.5, 0.5, 0.5]).tolist() == [1.0, 1.0, 1.0]
    assert significance.holm([0.2]).tolist() == [0.2]
    assert significance.holm([0.02, 0.02]).tolist() == [0.04, 0.04]                    # ties by index: 2 p, then max(2 p, p)
    g = np.random.default_rng(0)
    for m in (2, 8, 24):
        p = np.round(g.random(m), 2)
        assert np.array_equal(significance.holm(p), SI.holm_by_definition(p))
        assert np.all(significance.holm(p) >= p) and np.all(significance.holm(p) <= 1.0)


def test_mcnemar_against_binomtest_and_a_hand_case():
    from scipy.stats import binomtest
    from sm3hip import significance
    assert significance.mcnemar_p(1, 5) == significance.mcnemar_p(5, 1) == 14 / 64
    assert significance.mcnemar_p(0, 0) == 1.0 and significance.mcnemar_p(4, 4) == 1.0 and significance.mcnemar_p(0, 1) == 1.0
    for n10, n01 in ((0, 7), (3, 9), (10, 11), (40, 17), (300, 251), (4096, 4096), (1000, 7192)):
        got = significance.mcnemar_p(n10, n01)
        assert got == SI.mcnemar_exact(n10, n01)
        want = binomtest(min(n10, n01), n10 + n01, 0.5).pvalue
        assert abs(got - want) <= 1e-9 * want + 1e-300, (n10, n01, got, want)
    a, b, targets = SI.make_pair(129, "permuted", 4)
    res = significance.mcnemar(a, b, targets)
    ha, hb, y = SI.argmax(a), SI.argmax(b), targets.numpy()
    for t in range(8):
        n10 = int(((ha[:, t] == y[:, t]) & (hb[:, t] != y[:, t])).sum())
        n01 = int(((ha[:, t] != y[:, t]) & (hb[:, t] == y[:, t])).sum())
        assert (int(res["n10"][t]), int(res["n01"][t])) == (n10, n01) and float(res["p"][t]) == SI.mcnemar_exact(n10, n01)
    assert int(res["n10"][1:].sum()) == 0 and int(res["n10"][0]) + int(res["n01"][0]) > 0   # only label 0 was permuted
    assert np.array_equal(res["p_holm"].numpy(), SI.holm_by_definition(res["p"].numpy()))
    same = significance.mcnemar(a, a, targets)
    assert same["p"].tolist() == [1.0] * 8 and not same["n10"].any() and not same["n01"].any()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_in_order_before_any_device_work():
    from sm3hip import report, significance
    a, b, targets = SI.make_pair(5, "other", 1)
    other = targets.clone()
    other[2, 3] = (other[2, 3] + 1) % 3
    nan = [p.clone().fill_(float("nan")) if t == 2 else p for t, p in enumerate(b)]
    big = SI.make_pair(report.MAX_CASES + 1, "same", 1)
    big_nan = [p.clone().fill_(float("nan")) for p in big[0]]
    for fn in (significance.permutation_test, significance.delong, significance.mcnemar, significance.significance_report):
        with pytest.raises(ValueError, match="same cases"):                            # first: before the size limit
            fn(big_nan, big[1], big[2], targets_b=big[2][:-1])
        with pytest.raises(ValueError, match="same cases"):
            fn(a, b, targets, targets_b=other)
        with pytest.raises(ValueError, match=f"MAX_CASES = {report.MAX_CASES}"):       # then the limit: before NaN
            fn(big_nan, big[1], big[2], targets_b=big[2].clone())
        with pytest.raises(ValueError, match="NaN"):
            fn(a, nan, targets)
        with pytest.raises(ValueError):
            fn(a, b[:7], targets)
    for fn in (significance.permutation_test, significance.significance_report):
        with pytest.raises(ValueError, match="NaN"):                                   # NaN before the settings
            fn(a, nan, targets, permutations=0)
        for kw in ({"permutations": 0}, {"permutations": -1}, {"permutations": 1.5}, {"permutations": True},
                   {"permutations": 2 ** 24 + 1}, {"seed": -1}, {"seed": 2 ** 64}, {"seed": 0.5},
                   {"permutations": 4, "chunk": 0}, {"permutations": 4, "chunk": 5}, {"permutations": 4, "chunk": 2.0}):
            with pytest.raises(ValueError, match=next(iter(kw)) if len(kw) == 1 else "chunk"):
                fn(a, b, targets, **kw)
        with pytest.raises(ValueError, match="permutations"):                          # permutations before seed before chunk
            fn(a, b, targets, permutations=0, seed=-1, chunk=0)
        with pytest.raises(ValueError, match="seed"):
            fn(a, b, targets, permutations=4, seed=-1, chunk=0)
    for conf in (0.0, 1.0, True, "0.9"):
        with pytest.raises(ValueError, match="confidence"):
            significance.delong(a, b, targets, confidence=conf)
    before = [p.clone() for p in a + b] + [targets.clone()]
    significance.mcnemar(a, b, targets)
    assert all(torch.equal(p, q) for p, q in zip(a + b + [targets], before))


def test_the_tool_refuses_significance_without_against(capsys):
    er = _load("sm3_signif_cli_eval_report", os.path.join(TOOLS, "eval_report.py"))
    parser = er.get_parser()
    d = parser.parse_args(["x.pt"])
    assert (d.significance, d.permutations, d.permutation_seed) == (False, 10000, 0)
    s = parser.parse_args(["x.pt", "--against", "y.pt", "--significance", "--permutations", "500", "--permutation-seed", str(2 ** 63)])
    assert (s.significance, s.permutations, s.permutation_seed) == (True, 500, 2 ** 63)
    with pytest.raises(SystemExit) as e:                                               # no file is opened, no device touched
        er.main(["no_such_file.pt", "--significance"])
    assert e.value.code == 2 and "--against" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        er.main(["no_such_file.pt", "--against", "neither.pt", "--significance", "--permutations", "0"])
    assert e.value.code == 2 and "permutations" in capsys.readouterr().err
    import eval_cli
    assert all("signif" not in str(r) for r in eval_cli.REPORTS)                       # a comparison, not a per-tool report


# ---- 6. ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_stays_9_and_the_entry_points_refuse_bad_arguments_before_any_launch():
    from sm3hip import _lib, ops, report
    lib = _lib.load()
    assert lib.sm3_abi_version() == 9
    header = open(os.path.join(ROOT, "include", "sm3_hip.h")).read()
    for name in ("sm3_signif_counts", "sm3_signif_placements"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert callable(ops.signif_counts) and callable(ops.signif_placements)
    buf = (C.c_int64 * 1024)()
    p = C.cast(buf, C.c_void_p)  # host memory: never dereferenced, every call below returns before a launch
    odd = C.c_void_p(p.value + 4)

    def counts(order=p, gs=p, ge=p, y=p, ha=p, hb=p, colmap=p, out=p, N=5, T=8, K=24, seed=0, r0=0, c=1, point=0):
        return lib.sm3_signif_counts(order, gs, ge, y, ha, hb, colmap, out, N, T, K, seed, r0, c, point, None)
    for name in ("order", "gs", "ge", "y", "ha", "hb", "colmap", "out"):
        assert counts(**{name: None}) == -1, name
    assert counts(N=0) == -1 and counts(N=-3) == -1 and counts(N=report.MAX_CASES + 1) == -1
    assert counts(c=0) == -1 and counts(c=-1) == -1 and counts(point=1, c=2) == -1
    assert counts(T=0) == -1 and counts(T=65) == -1 and counts(K=0) == -1 and counts(K=65) == -1
    assert counts(r0=-1) == -1 and counts(r0=2 ** 32) == -1 and counts(r0=2 ** 32 - 1, c=2) == -1
    assert counts(out=odd) == -2

    def places(order=p, gs=p, ge=p, y=p, colmap=p, out=p, N=5, T=8, K=24):
        return lib.sm3_signif_placements(order, gs, ge, y, colmap, out, N, T, K, None)
    for name in ("order", "gs", "ge", "y", "colmap", "out"):
        assert places(**{name: None}) == -1, name
    assert places(N=0) == -1 and places(N=report.MAX_CASES + 1) == -1 and places(T=0) == -1 and places(K=65) == -1
    assert places(out=C.c_void_p(p.value + 2)) == -2
