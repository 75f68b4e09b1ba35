"""CPU: the proof that the GPU conditioning tests (test_norm_conditioning_gpu.py) can fail for the right reason.

On exactly the inputs those tests feed, the numpy models of the kernels' arithmetic (tests/norm_models.py) are held against
the same bounds: the shifted GroupNorm records and the two-pass LayerNorm statistics stay inside them, the same records with
the shift replaced by 0 and the one-pass E[x^2] - mean^2 miss them by at least 10x.  A kernel that lost its protection
against cancellation therefore cannot pass on the GPU."""
import pytest
import torch

import norm_models as nm


@pytest.mark.parametrize("eps", nm.GN_EPS)
@pytest.mark.parametrize("case", nm.GN_PARTIAL_CASES, ids=nm.case_id)
def test_shifted_records_hold_the_bounds_and_unshifted_records_miss_them(case, eps):
    n, hw, c0, c1 = case
    C = c0 + c1
    x = nm.gn_input(nm.GN_SEED, n, hw, C)
    gamma, beta = nm.affine(nm.GN_SEED + 1, C)
    coef, meanf, rstd = nm.gn_coef_model(x, 32, gamma, beta, eps, shifted=True)
    used, err = nm.check_coef(x, coef, 32, gamma, beta, eps)
    um, ur, ue = nm.check_group_stats(x, meanf, rstd, 32, eps)
    print(f"shifted:   coefficient planes use {used:.3f} of their bound (max error {err:.2e}); group mean {um:.3f}, rstd {ur:.3f}, "
          f"eps-dominated rstd {ue:.2e}")
    assert used <= 1.0 and um <= 1.0 and ur <= 1.0 and ue <= 1.0
    coef0, meanf0, rstd0 = nm.gn_coef_model(x, 32, gamma, beta, eps, shifted=False)
    used0, err0 = nm.check_coef(x, coef0, 32, gamma, beta, eps)
    _, ur0, ue0 = nm.check_group_stats(x, meanf0, rstd0, 32, eps)
    print(f"unshifted: coefficient planes use {used0:.1f} of their bound (max error {err0:.2e}); rstd {ur0:.0f}, eps-dominated rstd {ue0:.0f}")
    assert used0 >= 10.0, "the coefficient bound must tell the unshifted records from the shifted ones"
    assert ur0 >= 10.0 and ue0 >= 10.0, "so must the (mean, rstd) bounds of gn_group_stats"


@pytest.mark.parametrize("N", nm.GN_SITE_WIDTHS)
def test_tile_mean_records_hold_the_bound_on_biased_gemm_outputs_and_unshifted_records_miss_it(N):
    """The record-emitting GEMM epilogues are tested on outputs whose per-group offsets come from the bias: samples of 32 rows,
    unit-variance products.  The products themselves need the GPU; the same offsets on seeded noise of that shape stand in.
    A group then holds 32 x (1 .. 5) values, and next to the mean of a +0.3 group the coefficient bound is 2 .. 3 x 2^-24: records
    shifted by row 0 of the tile do not hold it (an outlier first row leaves partial sums of ~70 and 2 .. 6 x 2^-24 in the group
    mean; printed), records shifted by the tile's own mean -- what gn_tile_record, the igemm epilogues and the split-K reduce
    emit -- do."""
    x = nm.gn_input(nm.GN_SEED, 2, 32, N, special=False)
    gamma, beta = nm.affine(nm.GN_SEED + 1, N)
    used = {}
    for name, kw in (("tile mean", dict(tile_mean=True)), ("row 0", dict()), ("unshifted", dict(shifted=False))):
        coef, meanf, rstd = nm.gn_coef_model(x, 32, gamma, beta, 1e-5, **kw)
        used[name] = (nm.check_coef(x, coef, 32, gamma, beta, 1e-5)[0],) + nm.check_group_stats(x, meanf, rstd, 32, 1e-5, special=False)[:2]
        print(f"N = {N}, shift = {name}: coefficient planes use {used[name][0]:.3f} of their bound, group mean {used[name][1]:.3f}, rstd {used[name][2]:.3f}")
    assert max(used["tile mean"]) <= 1.0
    assert used["unshifted"][0] >= 10.0 and used["unshifted"][2] >= 10.0


@pytest.mark.parametrize("rows", nm.LN_ROWS)
@pytest.mark.parametrize("C", nm.LN_WIDTHS)
def test_two_pass_layernorm_holds_the_bounds_and_one_pass_misses_them(rows, C):
    x = nm.ln_input(nm.LN_SEED, rows, C)
    mean64, rstd64 = nm.ln_ref(x)
    lim = nm.ln_mean_limit(x, mean64)
    m2, r2 = nm.ln_stats_model(x, two_pass=True)
    m1, r1 = nm.ln_stats_model(x, two_pass=False)
    rel = lambda r: ((r.double() - rstd64) / rstd64).abs().max().item()
    print(f"rstd relative error: two-pass {rel(r2):.2e}, one-pass {rel(r1):.2e} (bound {nm.RSTD_REL:g}); "
          f"mean uses {((m2.double() - mean64).abs() / lim).max().item():.3f} of its limit")
    assert rel(r2) <= nm.RSTD_REL
    assert ((m2.double() - mean64).abs() <= lim).all()
    if C > 1:       # (a row of one element has variance 0 in every arithmetic: nothing to tell apart)
        assert rel(r1) >= 10 * nm.RSTD_REL, "the rstd bound must tell one-pass statistics from two-pass ones"


def test_inputs_are_what_they_claim():
    """Offsets constant inside a group and cycling over the groups; the constant and the tiny-variance group; the constant
    row; everything below the F16X2 range limit."""
    x = nm.gn_input(nm.GN_SEED, 2, 64, 160)
    g = x.reshape(2, 64, 32, 5)
    m, s = g.mean((1, 3)), g.std((1, 3))
    for k, off in enumerate(nm.OFFSETS):
        sel = [q for q in range(k, 32, 4) if q not in (nm.CONST_GROUP, nm.TINY_GROUP)]
        assert (m[:, sel] - off).abs().max() < 0.3 and (s[:, sel] - 1).abs().max() < 0.2
    assert (g[:, :, nm.CONST_GROUP] == nm.CONST_VALUE).all()
    assert (m[:, nm.TINY_GROUP] - 10).abs().max() < 1e-3 and 5e-4 < s[:, nm.TINY_GROUP].min() and s[:, nm.TINY_GROUP].max() < 2e-3
    r = nm.ln_input(nm.LN_SEED, 33, 320)
    assert (r[nm.CONST_ROW] == nm.CONST_VALUE).all() and abs(r[0].mean().item() - 100) < 0.3 and abs(r[3].mean().item() - 0.3) < 0.3
    assert max(x.abs().max().item(), r.abs().max().item()) < nm.F16X2_RANGE
    assert torch.equal(x, nm.gn_input(nm.GN_SEED, 2, 64, 160))
