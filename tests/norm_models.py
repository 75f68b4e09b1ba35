"""Shared pieces of the normalisation-conditioning tests (test_norm_models_cpu.py, test_norm_conditioning_gpu.py,
test_post_edges_gpu.py): the mean-dominated inputs, the float64 references, the error bounds, and numpy models of the
statistics kernels' arithmetic -- the GroupNorm partial-record format (csrc/norms.hip: gn_partial_kernel / gn_finalize_kernel,
csrc/ldmk_epilogue.h: gn_tile_record) carried out in float32 with and without the per-chunk shift, and the LayerNorm
statistics in their two-pass and one-pass forms.

The bounds are derived from the kernels' arithmetic (docstrings below), never from what a kernel returns; the CPU test
shows that the shifted / two-pass models stay inside them and the unshifted / one-pass models miss them by 10x or more on
exactly the inputs the GPU tests feed, so a GPU test that passes cannot have lost the cancellation protection."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rnd

U = 2.0 ** -24                          # unit roundoff of float32
F16X2_RANGE = 1000.0                    # LDMK_F16X2_RANGE (include/ldmk.h): every input here stays below it
OFFSETS = (100.0, -100.0, 30.0, 0.3)    # per-group (per-row) offsets, cycled; |mean| / std = 100, 100, 30, 0.3
CONST_GROUP, TINY_GROUP = 5, 10         # group 5: every element 3.7; group 10: 10 + 1e-3 z  (both eps-dominated)
CONST_VALUE = 3.7
SINGLE_ROW_OFFSET = 300.0
CONST_ROW = 7                           # LayerNorm inputs with more than CONST_ROW rows: this row is constant

# the cases the CPU models and the GPU kernels are both run on
GN_SEED, LN_SEED = 500, 520
GN_EPS = (1e-5, 1e-6)
GN_PARTIAL_CASES = [(2, 96, 64, 0),     # (n, hw, c0, c1): the plain case
                    (1, 40, 128, 0),    # last chunk holds 8 rows
                    (2, 64, 96, 64)]    # 5 channels per group; group 19 straddles the seam
GN_SITE_WIDTHS = (32, 64, 96, 160)      # output widths of the record-emitting GEMM / convolution cases (32 rows per sample)
LN_ROWS = (1, 33)
LN_WIDTHS = (1, 4, 16, 150, 192, 208, 320, 336, 640, 656, 1023, 1024, 1280)


def note(request, text):
    """One figure of the running test for its NORMCOND line (normcond_line prints them together when the test ends)."""
    request.node.__dict__.setdefault("_normcond", []).append(text)


@pytest.fixture(autouse=True)
def normcond_line(request):
    """Imported by the GPU test files: prints ONE line per test id, `NORMCOND <file>::<test id> <figure>; <figure>; ...` -- the
    lines profiles/norm_conditioning_errors.txt holds (pytest -s)."""
    yield
    parts = request.node.__dict__.get("_normcond")
    if parts:
        print(f"NORMCOND {request.node.nodeid.split('/')[-1]} " + "; ".join(parts))


def case_id(case):
    return "x".join(str(v) for v in case)


# ---------------------------------------------------------------------------------------------- inputs
def group_offsets(C, groups=32):
    """[C] offset of each channel: constant inside a group, OFFSETS cycled over the groups."""
    cpg = C // groups
    return torch.tensor([OFFSETS[(c // cpg) % len(OFFSETS)] for c in range(C)], dtype=torch.float32)


def gn_input(seed, n, hw, C, groups=32, special=True):
    """[n][hw][C] float32: unit-variance noise plus the per-group offsets; with `special`, group CONST_GROUP is exactly
    constant and group TINY_GROUP has variance 1e-6 around 10."""
    z = rnd(seed, n, hw, C)
    x = z + group_offsets(C, groups)
    if special:
        cpg = C // groups
        x[..., CONST_GROUP * cpg:(CONST_GROUP + 1) * cpg] = CONST_VALUE
        t = slice(TINY_GROUP * cpg, (TINY_GROUP + 1) * cpg)
        x[..., t] = 10.0 + 1e-3 * z[..., t]
    assert x.abs().max().item() < F16X2_RANGE
    return x.contiguous()


def eps_dominated_groups(groups=32):
    m = torch.zeros(groups, dtype=torch.bool)
    m[CONST_GROUP] = m[TINY_GROUP] = True
    return m


def ln_input(seed, rows, C):
    """[rows][C] float32 token rows: unit-variance noise plus one offset per row (OFFSETS cycled); row CONST_ROW constant.
    A single row is a single draw of the one-pass error, which a lucky draw keeps small at offset 100: it gets offset 300."""
    offs = [OFFSETS[r % len(OFFSETS)] for r in range(rows)] if rows > 1 else [SINGLE_ROW_OFFSET]
    x = rnd(seed, rows, C) + torch.tensor(offs, dtype=torch.float32)[:, None]
    if rows > CONST_ROW:
        x[CONST_ROW] = CONST_VALUE
    assert x.abs().max().item() < F16X2_RANGE
    return x.contiguous()


def affine(seed, C):
    """(gamma, beta) as the other tests make them."""
    return 1 + 0.1 * rnd(seed, C), 0.1 * rnd(seed + 1, C)


# ---------------------------------------------------------------------------------------------- float64 references
def gn_ref(x, groups, gamma, beta, eps):
    """float64 GroupNorm of the stored float32 tensor x [n][hw][C] (channel-last) -> (y [n][hw][C], mean [n][groups],
    rstd [n][groups]); y is F.group_norm itself, mean / rstd are the group values it used."""
    n, hw, C = x.shape
    xd = x.double()
    y = F.group_norm(xd.permute(0, 2, 1), groups, gamma.double(), beta.double(), eps).permute(0, 2, 1)
    g = xd.reshape(n, hw, groups, C // groups)
    mean = g.mean((1, 3))
    var = ((g - mean[:, None, :, None]) ** 2).mean((1, 3))
    return y, mean, 1.0 / torch.sqrt(var + eps)


def ln_ref(x, eps=1e-5):
    """float64 (mean, rstd) per row of the float32 matrix x."""
    xd = x.double()
    mean = xd.mean(1)
    return mean, 1.0 / torch.sqrt(((xd - mean[:, None]) ** 2).mean(1) + eps)


# ---------------------------------------------------------------------------------------------- bounds
def gn_coef_bound(x, mean, rstd, gamma, groups=32):
    """Per-element bound [n][hw][C] on |x*coef[0] + coef[1] - GroupNorm64(x)| with fp32 coefficient planes:
        8 * 2^-24 * (|mean_g| rstd_g + |xhat|) * max|gamma|.
    One rounding each for rstd, sc = rstd*gamma, meanf and sh = fma(-meanf, sc, beta), each worth at most
    2^-24 |mean_g| rstd_g |gamma| in y, plus 2 * 2^-24 |x sc| <= 2 * 2^-24 (|mean_g| rstd_g + |xhat|) |gamma| for the
    representation of the two planes' product with x: about 6, rounded up to 8."""
    n, hw, C = x.shape
    cpg = C // groups
    m, r = mean.repeat_interleave(cpg, 1)[:, None, :], rstd.repeat_interleave(cpg, 1)[:, None, :]
    xhat = (x.double() - m) * r
    return 8 * U * (m.abs() * r + xhat.abs()) * gamma.abs().max().item()


def gn_out_bound(x, mean, rstd, gamma, y, groups=32):
    """Normalised outputs a kernel writes itself (ldmk_post norm_out): the coefficient bound plus 4 * 2^-24 |y| for the
    output's own fp32 arithmetic ((v - mean) * rstd, the fma with gamma / beta, the store)."""
    return gn_coef_bound(x, mean, rstd, gamma, groups) + 4 * U * y.abs()


def group_mean_bound(mean):
    return 2.0 ** -23 * mean.abs() + 1e-6


RSTD_REL = 2e-6                         # (mean, rstd) producers: relative rstd error, the bound of test_ps_gpu.py
RSTD_REL_EPS_DOMINATED = 1e-4           # constant / tiny-variance groups: rstd ~ eps^-1/2, checked against float64 at 1e-4


def ln_mean_limit(x, mean64):
    """Per-row limit on the LayerNorm mean: 4 x the worst error torch's own fp32 row mean makes on the same input (the
    kernels sum 8 or 32 per-lane chains plus shuffles, an order torch does not use), floored at 2^-22 max(1, |mean|)."""
    torch_err = (x.mean(1).double() - mean64).abs().max().item()
    return torch.clamp(2.0 ** -22 * torch.clamp(mean64.abs(), min=1.0), min=4 * torch_err)


def ln_out_bound(x, mean, rstd, gamma, y):
    """LayerNorm outputs written directly (ldmk_ln_apply, ldmk_post LayerNorm): the coefficient bound with the row in the
    place of the group, plus 4 * 2^-24 |y|."""
    m, r = mean[:, None], rstd[:, None]
    xhat = (x.double() - m) * r
    return 8 * U * (m.abs() * r + xhat.abs()) * gamma.abs().max().item() + 4 * U * y.abs()


# ---------------------------------------------------------------------------------------------- numpy models
def _f32(a):
    return np.asarray(a, dtype=np.float32)


def gn_records(x, shifted=True, tile_mean=False):
    """The partial records of x [n][hw][C] in float32: [n][chunks][C][3] = (shift, sum(x - shift), sum (x - shift)^2) per
    32-row chunk and column.  shift = row 0 of the chunk (gn_partial_kernel, the Winograd / upsampling output transforms) or, with
    `tile_mean`, the fp32 mean of the chunk (gn_tile_record, the igemm epilogues and the split-K reduce, which hold the 32 values
    in registers / LDS); shifted=False: shift 0, the naive sums."""
    xn = x.numpy() if isinstance(x, torch.Tensor) else x
    n, hw, C = xn.shape
    chunks = (hw + 31) // 32
    rec = np.zeros((n, chunks, C, 3), np.float32)
    for k in range(chunks):
        blk = xn[:, k * 32:(k + 1) * 32]
        if not shifted:
            sh = np.zeros((n, C), np.float32)
        elif tile_mean:
            sh = np.zeros((n, C), np.float32)
            for r in range(blk.shape[1]):
                sh = _f32(sh + blk[:, r])
            sh = _f32(sh * np.float32(1.0 / blk.shape[1]))
        else:
            sh = blk[:, 0].copy()
        s, ss = np.zeros((n, C), np.float32), np.zeros((n, C), np.float32)
        for r in range(blk.shape[1]):
            v = _f32(blk[:, r] - sh)
            s = _f32(s + v)
            ss = _f32(v.astype(np.float64) * v + ss)            # fmaf(v, v, ss): one rounding
        rec[:, k, :, 0], rec[:, k, :, 1], rec[:, k, :, 2] = sh, s, ss
    return rec


def gn_finalize(rec, hw, groups, eps):
    """gn_finalize_kernel / gn_group_stats: un-shift and combine in float64 -> (meanf [n][groups] float32, rstd float32)."""
    n, chunks, C, _ = rec.shape
    cnt = np.minimum(hw - 32 * np.arange(chunks), 32).astype(np.float64)[None, :, None]
    sh, s, ss = (rec[..., i].astype(np.float64) for i in range(3))
    S = (s + cnt * sh).sum(1)
    Q = (ss + 2.0 * sh * s + cnt * sh * sh).sum(1)
    cpg = C // groups
    Sg, Qg = S.reshape(n, groups, cpg).sum(2), Q.reshape(n, groups, cpg).sum(2)
    mean = Sg / (cpg * hw)
    var = np.maximum(Qg / (cpg * hw) - mean * mean, 0.0)
    return _f32(mean), _f32(1.0 / np.sqrt(var + eps))


def gn_coef_model(x, groups, gamma, beta, eps, shifted=True, tile_mean=False):
    """The coefficient planes [n][2][C] (float32) the record format yields: sc = rstd*gamma, sh = fma(-meanf, sc, beta)."""
    n, hw, C = x.shape
    meanf, rstd = gn_finalize(gn_records(x, shifted, tile_mean), hw, groups, eps)
    cpg = C // groups
    sc = _f32(np.repeat(rstd, cpg, 1) * _f32(gamma.numpy()))
    sh = _f32(-np.repeat(meanf, cpg, 1).astype(np.float64) * sc + _f32(beta.numpy()).astype(np.float64))
    return torch.from_numpy(np.stack([sc, sh], 1)), torch.from_numpy(meanf), torch.from_numpy(rstd)


def apply_coef(x, coef):
    """y = x*coef[0] + coef[1] in float64 from float32 planes [n][2][C] and the float32 tensor x [n][hw][C]."""
    c = coef.double().cpu()
    return x.double().cpu() * c[:, 0][:, None, :] + c[:, 1][:, None, :]


def ln_stats_model(x, eps=1e-5, two_pass=True):
    """float32 LayerNorm (mean, rstd) per row: two-pass (centred squares, what the kernels do in registers) or one-pass
    E[x^2] - mean^2."""
    xn = x.numpy()
    C = xn.shape[1]
    mean = _f32(xn.sum(1, dtype=np.float32) / np.float32(C))
    if two_pass:
        d = _f32(xn - mean[:, None])
        var = _f32(_f32(d * d).sum(1, dtype=np.float32) / np.float32(C))
    else:
        var = _f32(_f32(xn * xn).sum(1, dtype=np.float32) / np.float32(C)) - _f32(mean * mean)
        var = np.maximum(_f32(var), np.float32(0))
    rstd = _f32(1.0 / np.sqrt(_f32(var + np.float32(eps))))
    return torch.from_numpy(mean), torch.from_numpy(rstd)


# ---------------------------------------------------------------------------------------------- checks shared by CPU and GPU tests
def check_coef(x, coef, groups, gamma, beta, eps, detail=False):
    """(worst |error| / bound over the elements, worst |error|) of coefficient planes against float64 GroupNorm of x; with
    `detail` also a description of the worst element (its group's mean and rstd, its xhat, the error in units of 2^-24)."""
    y64, mean, rstd = gn_ref(x, groups, gamma, beta, eps)
    err = (apply_coef(x, coef) - y64).abs()
    used = err / gn_coef_bound(x, mean, rstd, gamma, groups)
    if not detail:
        return used.max().item(), err.max().item()
    i, p_, c = np.unravel_index(used.argmax().item(), used.shape)
    g = c // (x.shape[-1] // groups)
    where = (f"worst element: sample {i} row {p_} channel {c} (group {g}: mean {mean[i, g].item():.4g}, rstd {rstd[i, g].item():.4g}), "
             f"xhat {((x[i, p_, c].item() - mean[i, g].item()) * rstd[i, g].item()):.3g}, beta {beta[c].item():.3g}, "
             f"error {err[i, p_, c].item() / U:.2f} x 2^-24")
    return used.max().item(), err.max().item(), where


def check_group_stats(x, meanf, rstdf, groups, eps, special=True):
    """Worst used fraction of the (mean, rstd) bounds of gn_group_stats: (mean, rstd outside the eps-dominated groups, rstd
    inside them).  In the constant and the tiny-variance group rstd is eps^-1/2 to within the absolute error of a variance
    that is (next to) zero: checked against float64 at relative 1e-4 there."""
    C = x.shape[-1]
    _, mean, rstd = gn_ref(x, groups, torch.ones(C), torch.zeros(C), eps)
    um = ((meanf.double().cpu() - mean).abs() / group_mean_bound(mean)).max().item()
    rel = ((rstdf.double().cpu() - rstd) / rstd).abs()
    dom = eps_dominated_groups(groups)[None, :].expand_as(rel) if special else torch.zeros_like(rel, dtype=torch.bool)
    ur = (rel[~dom] / RSTD_REL).max().item()
    ue = (rel[dom] / RSTD_REL_EPS_DOMINATED).max().item() if dom.any() else 0.0
    return um, ur, ue
