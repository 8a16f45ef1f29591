"""CPU: the references and bounds of the edge suites, checked without the library.

The GPU edge suites (test_ntxent_edges_gpu.py, test_optimizer_edges_gpu.py, test_augment_edges_gpu.py) hold kernels to
bounds against fp64.  Here the same formulas run in torch fp32 on the same inputs (tests/edge_inputs.py) and must stay
within a fraction of each bound: half for AdamW and NT-Xent, a quarter for the colour ops.  A bound that fp32
arithmetic alone could not meet would say nothing about a kernel."""
import math

import numpy as np
import pytest
import torch

import edge_inputs as E
from oracle import augment_oracle as A
from oracle import sm3_oracle as O


@pytest.mark.parametrize("R,D", [s for s in E.NTX_SHAPES if s[0] <= 130], ids=str)
def test_ntxent_bounds_are_met_by_an_fp32_restatement(R, D):
    worst_l = worst_d = 0.0
    for T in E.NTX_TEMPS:
        for scaled in (False, True):
            z = E.clustered(R, D, seed=R * 1000 + D, row_scale=scaled)
            ref_l, ref_g = E.ntxent_ref(z, T)
            got_l, got_g = E.ntxent_f32(z, T)
            worst_l = max(worst_l, abs(got_l - ref_l) / E.loss_limit(ref_l))
            worst_d = max(worst_d, E.worst_ratio(got_g, ref_g, E.dz_limit(ref_g)))
    assert worst_l <= 0.5 and worst_d <= 0.5, (worst_l, worst_d)


def test_clustered_inputs_have_the_cosines_they_claim():
    z = E.clustered(130, 128, seed=1).double()
    zn = z / z.norm(dim=1, keepdim=True)
    s = zn @ zn.t()
    B = 65
    pos = s[torch.arange(B), torch.arange(B) + B]
    assert float(pos.min()) > 0.999
    same = s[0, 3]  # pairs 0 and 3 share centre 0
    assert 0.98 < float(same) < 0.9995
    # at T = 0.01 the logits reach +-100: exp() of them overflows fp32 unless the maximum is subtracted
    assert float(s.max()) / 0.01 > math.log(np.finfo(np.float32).max)
    sc = E.clustered(130, 128, seed=1, row_scale=True).double().norm(dim=1)
    assert float(sc.max() / sc.min()) > 1e5


def test_oracle_handles_a_zero_row_and_an_exact_duplicate():
    """F.normalize's clamp: a zero row has zn = 0 and passes its gradient through 1 / 1e-12; no NaN."""
    z = E.clustered(10, 36, seed=5)
    z[3] = 0
    loss, g = E.ntxent_ref(z, 0.07)
    assert math.isfinite(loss) and bool(torch.isfinite(g).all()) and float(g[3].abs().max()) > 1e6
    z = E.clustered(10, 36, seed=5)
    z[1] = z[0]
    loss, g = E.ntxent_ref(z, 0.07)
    assert math.isfinite(loss) and bool(torch.isfinite(g).all())


def test_rect_restatement_on_cosines_is_the_oracle():
    zl = E.clustered(6, 36, seed=2).double()
    za = torch.cat([E.clustered(6, 36, seed=3).double(), zl, E.clustered(6, 36, seed=4).double()])
    nrm = lambda t: t / t.norm(dim=1, keepdim=True)
    S = nrm(zl) @ nrm(za).t()
    assert abs(float(E.rect_loss_from_s(S, 6, 0.07)) - float(O.ntxent_global_rows(zl, za, 6, 0.07))) < 1e-12


@pytest.mark.parametrize("grad_scale,wd", [(1.0, 0.05), (0.125, 0.05), (1.0, 0.0), (0.125, 0.0)])
def test_adamw_bounds_are_met_by_an_fp32_restatement(grad_scale, wd):
    n = 200003
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(1))
    grads = E.adamw_grads(n, 5, seed=2)
    pr, mr, vr = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    gsum = torch.zeros(n, dtype=torch.float64)
    for step, g in enumerate(grads, start=1):
        E.adamw_ref_step(pr, g.double(), mr, vr, step, wd, grad_scale)
        E.adamw_f32_step(p, g, m, v, step, wd, grad_scale)
        gsum += (g.double() * grad_scale).abs()
    rp, rm, rv = E.adamw_ratios("cpu fp32", p, m, v, pr, mr, vr, gsum)
    assert rp <= 0.5 and rm <= 0.5 and rv <= 0.5, (rp, rm, rv)


def test_adamw_tuples_hold_the_edge_values():
    p, g, m, v = E.adamw_tuples()
    assert p.numel() == 37 and len({t for t in zip(p.tolist(), g.tolist(), m.tolist(), v.tolist())}) == 37
    assert math.copysign(1.0, float(p[1])) == -1.0 and float(p[2]) > 0 and float(p[3]) > 1e29
    assert {0.0, E.f32(1e-20), 1e4} <= set(g.tolist()) and 0.0 in v.tolist()


def test_pixel_table_holds_what_the_colour_tests_rely_on():
    t = E.pixel_table()
    assert t.shape[1] == 3 and t.shape[0] == 216 + 120 + 3000 and float(t.min()) == 0.0 and float(t.max()) == 1.0
    rows = {tuple(r) for r in t.tolist()}
    assert (0.0, 0.0, 0.0) in rows and (1.0, 1.0, 1.0) in rows and (1.0, 0.0, 0.0) in rows
    one_ulp = (1.0, E.f32(1.0 - 2.0 ** -24), E.f32(1.0 - 2.0 ** -23))
    assert one_ulp in rows and one_ulp[1] < 1.0
    for H, W in E.AUG_SIZES:  # every pixel of the table occurs at every image size
        img = E.table_images(H, W)
        assert {tuple(r) for r in img.permute(0, 2, 3, 1).reshape(-1, 3).tolist()} == rows


def test_colour_bounds_are_met_by_the_oracle_in_fp32():
    """The oracle in fp32 against itself in fp64, on the GPU tests' own pixels: a quarter of each bound at the most."""
    worst = 0.0
    img = E.table_images(61, 54)
    for op, factors in E.AUG_FACTORS.items():
        for f in factors:
            d = (E.color_ref(img, op, f, torch.float32).double() - E.color_ref(img, op, f)).abs().max()
            worst = max(worst, float(d))
    assert worst <= E.AUG_OP_LIMIT / 4, worst
    ops, fac = E.draw_chains(50, seed=50)
    img = E.table_images(61, 54, B=50, seed=9)
    d = float((E.chain_ref(img, ops, fac, torch.float32).double() - E.chain_ref(img, ops, fac)).abs().max())
    assert d <= E.AUG_CHAIN_LIMIT / 4, d


def test_hue_round_trip_is_continuous_at_ties_and_sector_borders():
    """No discontinuity allowance is needed: a 1-ulp change of one channel moves the hue-shifted pixel by ~1 ulp."""
    t = E.pixel_table().double()
    img = t.t().reshape(3, 1, -1)
    for f in E.AUG_FACTORS[4]:
        base = A.color_op(img, 4, E.f32(f))
        for c in range(3):
            bumped = img.clone()
            bumped[c] = (bumped[c] + 2.0 ** -24).clamp(0, 1)
            assert float((A.color_op(bumped, 4, E.f32(f)) - base).abs().max()) < 1e-6
