"""GPU: every statistics producer of the GroupNorm / LayerNorm split on MEAN-DOMINATED data (|mean| / std up to 100, an
exactly constant group and a tiny-variance group: tests/norm_models.py), against float64 of the tensor actually stored.

The producers keep a per-chunk shift in their records and un-shift in double (GroupNorm) or take the centred second moment
in registers (LayerNorm).  At |mean| / std of 0.2-0.4, which is what every other test feeds, a kernel without that protection
passes the 1e-5 tolerances; here it misses the bounds by 10x or more (shown without a GPU in test_norm_models_cpu.py on the
same inputs).  The bounds come from the arithmetic (norm_models.gn_coef_bound & co.), never from the kernels."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_models as nm
from conftest import rnd
from norm_models import normcond_line  # noqa: F401  (autouse: one NORMCOND line per test id)
from test_ops_gpu import nhwc, ops  # noqa: F401  (the `ops` fixture)
from test_ps_gpu import _split3

pytestmark = pytest.mark.gpu


def _report(request, what, err, used):
    nm.note(request, f"{what}: max error {err:.3e}, {used:.3f} of its bound")


def _check_records(ops, request, stored, parts, widths, n, hw, eps, special):
    """Coefficient planes (ldmk_gn_finalize) and group statistics (ldmk_gn_group_stats) from partial records `parts` (one or two
    tensors of the channel concat, widths (c0, c1)) against float64 GroupNorm of `stored` [n][hw][C] (CPU float32)."""
    from dsml_thesis_amd import lib as L, train_ops as T
    c0, c1 = widths
    Cc = c0 + c1
    gamma, beta = nm.affine(nm.GN_SEED + 1, Cc)
    gd, bd = gamma.cuda(), beta.cuda()
    coef = torch.empty(n, 2, Cc, device="cuda")
    p1 = parts[1] if c1 else None
    L.call("ldmk_gn_finalize", parts[0].data_ptr(), c0, None if p1 is None else p1.data_ptr(), c1, n, hw, 32, eps, gd.data_ptr(),
           bd.data_ptr(), coef.data_ptr(), ops.stream())
    mr = T.gn_group_stats(parts[0], c0, p1, c1, n, hw, 32, eps)
    used, err, where = nm.check_coef(stored, coef.cpu(), 32, gamma, beta, eps, detail=True)
    um, ur, ue = nm.check_group_stats(stored, mr[..., 0], mr[..., 1], 32, eps, special)
    _report(request, "coefficient planes", err, used)
    nm.note(request, where)
    nm.note(request, f"group stats: mean {um:.3f}, rstd {ur:.3f}, eps-dominated rstd {ue:.3f} of their bounds")
    assert used <= 1.0, f"coefficient planes use {used:.3f} of their bound (max error {err:.3e})"
    assert um <= 1.0 and ur <= 1.0 and ue <= 1.0, (um, ur, ue)
    return coef, mr


# ---- (a) the stand-alone statistics pass ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", nm.GN_EPS)
@pytest.mark.parametrize("case", nm.GN_PARTIAL_CASES, ids=nm.case_id)
def test_gn_partial_records_on_mean_dominated_groups(ops, request, case, eps):
    from dsml_thesis_amd import lib as L
    n, hw, c0, c1 = case
    x = nm.gn_input(nm.GN_SEED, n, hw, c0 + c1)
    chunks = L.load().ldmk_gn_chunks(hw)
    srcs = [x[..., :c0].contiguous().cuda()] + ([x[..., c0:].contiguous().cuda()] if c1 else [])
    parts = []
    for s in srcs:
        p = torch.empty(n * chunks * s.shape[-1] * 3, device="cuda")
        L.call("ldmk_gn_partial", s.data_ptr(), s.shape[-1], n, hw, p.data_ptr(), ops.stream())
        parts.append(p)
    _check_records(ops, request, x, parts, (c0, c1), n, hw, eps, special=True)


# ---- (b) one case per record-emitting code site; the per-group offsets ride in the bias, the product has unit variance ----------------
# With 32 rows per sample a group holds 32 x (1 .. 5) values, and next to the mean of a +0.3 group (xhat ~ 0, |mean_g| rstd_g ~ 0.2 .. 0.3)
# the coefficient bound is 2 .. 3 x 2^-24 in y.  Records shifted by row 0 of the tile missed it at two sites (1.32 of the bound from the
# split-K reduce, 1.13 from tile_cfg 12; 0.99 from tile_cfg 4): an outlier first row leaves partial sums of ~70 in sum(x - shift) and
# 2 .. 6 x 2^-24 in the group mean.  These sites hold the tile's 32 values in registers / LDS and now shift by the tile's own mean.
def _gemm_operands(ops, M, K, N):
    x, w = rnd(530, M, K), rnd(531, N, K) / np.sqrt(K)
    return x.cuda(), ops.pack_linear(w.cuda()), nm.group_offsets(N).cuda()


def _igemm_site(ops, request, M, K, N, prepare, **kw):
    """rows-mode GEMM with rows_per_sample = 32 (M / 32 samples in one launch) and stats_out; `prepare(x, wp)` -> extra arguments"""
    from dsml_thesis_amd import lib as L
    x, wp, bias = _gemm_operands(ops, M, K, N)
    extra = prepare(x, wp) if prepare else {}
    a0 = None if "a_ps" in extra else x
    out = torch.empty(M, N, device="cuda")
    rec = torch.zeros(M // 32, N, 3, device="cuda")
    a = ops.make_igemm_args(M, N, K, a0, K, wp, out, N, 32, bias=bias, **extra, **kw)
    a.stats_out = rec.data_ptr()
    assert L.load().ldmk_igemm_check(C.byref(a)) == 0, L.load().ldmk_last_error()
    ops.igemm(a)
    flag = extra.get("range_flag")
    assert flag is None or int(flag.item()) == 0, "values stay below LDMK_F16X2_RANGE"
    ref = x.double().cpu() @ wp.double().cpu() + bias.double().cpu()
    torch.testing.assert_close(out.cpu().double(), ref, rtol=1e-4, atol=1e-4)
    _check_records(ops, request, out.cpu().reshape(M // 32, 32, N), [rec], (N, 0), M // 32, 32, 1e-5, special=False)


def _flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("M,N", [(64, 64), (96, 96)])
def test_records_lds_tiled_igemm(ops, request, M, N):
    """tile_cfg 4 (64x64): whole tiles take the lean epilogue, the ragged tiles of the 96x96 problem the general one"""
    _igemm_site(ops, request, M, 64, N, None, tile_cfg=4, splitk=1)


@pytest.mark.parametrize("counters", [False, True])
def test_records_split_k_reduce_and_in_launch_combine(ops, request, counters):
    """The reduce launch (counters off) and the in-launch combine (counters on) of a 2-way K split."""
    ws = torch.empty(2 * 96 * 96, device="cuda")
    cnt = torch.zeros(1024, dtype=torch.int32, device="cuda") if counters else None
    _igemm_site(ops, request, 96, 128, 96, None, tile_cfg=4, splitk=2, splitk_ws=ws, splitk_counters=cnt)
    assert cnt is None or int(cnt.abs().sum()) == 0


@pytest.mark.parametrize("cfg", [12, 13])
def test_records_row_gemm_and_slab_gemm(ops, request, cfg):
    """tile_cfg 12 (csrc/rgemm.hip) and 13 (csrc/sgemm.hip): gn_tile_record from their own epilogues"""
    ws = torch.empty(64 * 64 + 8, device="cuda")
    _igemm_site(ops, request, 64, 64, 64, lambda x, wp: dict(w_frag=ops.pack_wfrag(wp)), tile_cfg=cfg, splitk=1, splitk_ws=ws)


def test_records_warp_specialised_tile(ops, request):
    from dsml_thesis_amd import lib as L

    def prepare(x, wp):
        ops.pack_wsplit(wp)      # registers the bf16x3 images of wp, keyed by its address: make_igemm_args(compute=BF16X3) finds them there
        return {}
    _igemm_site(ops, request, 64, 64, 128, prepare, tile_cfg=22, splitk=1, compute=L.COMPUTE_BF16X3)


@pytest.mark.parametrize("h2", [False, True], ids=["bf16x3", "f16x2"])
def test_records_pre_split_rows_tile(ops, request, h2):
    def prepare(x, wp):
        if not h2:
            return dict(a_ps=ops.pack_ps(x), w_ps=ops.pack_wps(wp))
        flag = _flag()
        return dict(a_ps=ops.pack_ps(x, h2_flag=flag), w_ps=ops.pack_wps(wp, h2=True), range_flag=flag)
    _igemm_site(ops, request, 64, 64, 160, prepare, tile_cfg=27, splitk=1)


def _conv_operands(n, cin, cout, h, w):
    x, wt = rnd(540, n, cin, h, w), rnd(541, cout, cin, 3, 3) / np.sqrt(9 * cin)
    return x, wt, nm.group_offsets(cout)


def _check_conv(ops, request, y, rec, ref, n, hw, cout):
    torch.testing.assert_close(y.cpu().double().reshape(n, hw, cout), ref.permute(0, 2, 3, 1).reshape(n, hw, cout), rtol=1e-4, atol=1e-4)
    _check_records(ops, request, y.cpu().reshape(n, hw, cout), [rec], (cout, 0), n, hw, 1e-5, special=False)


def test_records_conv_mode_pre_split_tile(ops, request):
    n, cin, cout, h, w = 2, 32, 64, 8, 8
    x, wt, b = _conv_operands(n, cin, cout, h, w)
    wp = ops.pack_conv3x3(wt.cuda())
    flag = _flag()
    yps = ops.pack_ps(nhwc(x).reshape(n * h * w, cin), h2_flag=flag)
    rec = torch.zeros(n * h * w // 32, cout, 3, device="cuda")
    y = ops.conv3x3_ps(yps, n, h, w, cin, wp, ops.pack_wps(wp, h2=True), flag, bias=b.cuda(), tile_cfg=27, stats_out=rec)
    assert int(flag.item()) == 0
    _check_conv(ops, request, y, rec, F.conv2d(x.double(), wt.double(), b.double(), padding=1), n, h * w, cout)


# The two output transforms below (like ldmk_gn_partial) stream their rows and shift by the first value they see, not by the chunk
# mean.  The coefficient bound is not guaranteed for that form at small groups (norm_models: 0.53 .. 1.63 of it at 32 .. 160 values per
# group); the shapes the cases call for give groups of 128 and 512 values.
def test_records_winograd_output(ops, request):
    n, cin, cout, h, w = 2, 32, 64, 8, 8
    x, wt, b = _conv_operands(n, cin, cout, h, w)
    rec = torch.zeros(n * h * w // 32, cout, 3, device="cuda")
    y = ops.conv3x3_winograd(nhwc(x), ops.pack_winograd(wt.cuda()), bias=b.cuda(), stats_out=rec)
    _check_conv(ops, request, y, rec, F.conv2d(x.double(), wt.double(), b.double(), padding=1), n, h * w, cout)


def test_records_upconv_scatter(ops, request):
    n, cin, cout, h, w = 1, 32, 64, 4, 16
    x, wt, b = _conv_operands(n, cin, cout, h, w)
    rec = torch.zeros(n * 4 * h * w // 32, cout, 3, device="cuda")
    y = ops.upsample_conv3x3_phases(nhwc(x), ops.pack_upconv(wt.cuda()), b.cuda(), stats_out=rec)
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), wt.double(), b.double(), padding=1)
    _check_conv(ops, request, y, rec, ref, n, 4 * h * w, cout)


# ---- (c) LayerNorm statistics -----------------------------------------------------------------------------------------------------------
def _check_ln_stats(request, st, x, what):
    mean64, rstd64 = nm.ln_ref(x)
    st = st.cpu().double()
    merr, lim = (st[:, 0] - mean64).abs(), nm.ln_mean_limit(x, mean64)
    rel = ((st[:, 1] - rstd64) / rstd64).abs().max().item()
    nm.note(request, f"{what}: rstd relative error {rel:.3e} ({rel / nm.RSTD_REL:.3f} of its bound), "
          f"mean error {merr.max().item():.3e} ({(merr / lim).max().item():.3f} of its limit)")
    assert rel <= nm.RSTD_REL, f"{what}: rstd relative error {rel:.3e}"
    assert (merr <= lim).all(), f"{what}: mean error {merr.max().item():.3e} uses {(merr / lim).max().item():.3f} of its limit"


@pytest.mark.parametrize("rows", nm.LN_ROWS)
@pytest.mark.parametrize("Cw", [4, 320, 1024, 1, 150, 1023])
def test_ln_stats_on_mean_dominated_rows(ops, request, Cw, rows):
    """the float4 kernel (C % 4 == 0) at its narrowest and widest, the scalar kernel at C = 1, 150 and 1023"""
    x = nm.ln_input(nm.LN_SEED, rows, Cw)
    _check_ln_stats(request, ops.ln_stats(x.cuda()), x, "ldmk_ln_stats")


@pytest.mark.parametrize("rows", nm.LN_ROWS)
def test_ln_stats_split_on_mean_dominated_rows(ops, request, rows):
    Cw = 320
    x = nm.ln_input(nm.LN_SEED, rows, Cw)
    split = torch.zeros(3, rows, Cw, dtype=torch.bfloat16, device="cuda")
    _check_ln_stats(request, ops.ln_stats(x.cuda(), split=split), x, "ldmk_ln_stats_split")
    for img, want in zip(split.float().cpu(), _split3(x)):
        assert torch.equal(img, want), "the images are the exact three-way split"


@pytest.mark.parametrize("h2", [False, True], ids=["bf16x3", "f16x2"])
@pytest.mark.parametrize("rows", nm.LN_ROWS)
@pytest.mark.parametrize("Cw", [16, 192, 208, 320, 336, 640, 656, 1280])
def test_ln_stats_ps_on_mean_dominated_rows(ops, request, Cw, rows, h2):
    """both sides of every template boundary of ln_stats_ps_kernel (C <= 192 / 320 / 640 / 1280) and C = 16"""
    x = nm.ln_input(nm.LN_SEED, rows, Cw)
    xc = x.cuda()
    for guard, want in ((4.0, 1), (1e9, 0)):
        flag, rflag = _flag(), _flag()
        st, ps = ops.ln_stats_ps(xc, guard=guard, flag=flag, h2_flag=rflag if h2 else None)
        assert int(flag.item()) == want, f"guard {guard:g}: every row here has |mean| * rstd >= 30 or is constant"
        assert int(rflag.item()) == 0, "values stay below LDMK_F16X2_RANGE"
        assert torch.equal(ps, ops.pack_ps(xc, h2_flag=_flag() if h2 else None)), "the planes are pack_ps of the rows"
    _check_ln_stats(request, st, x, "ldmk_ln_stats_ps_h2" if h2 else "ldmk_ln_stats_ps")


# ---- (d) the backward consumers on the same mean-dominated x --------------------------------------------------------------------------
def _measure(got, ref):
    """the measure of test_backward_gpu._close: max error over max |reference|"""
    ref = ref.detach().double().cpu()
    return (got.detach().double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _autograd(fn, inputs, dy, dtype):
    leaves = [v.to(dtype).requires_grad_(True) for v in inputs]
    with torch.enable_grad():
        y = fn(*leaves)
        y.backward(dy.to(dtype))
    return [y.detach()] + [v.grad for v in leaves]


def _limits(fn, inputs, dy, floor):
    """float64 autograd of fn, and per result the limit: 4 x the error fp32 CPU autograd of the same graph shows against it
    (measured against the fp32 reference, never against the kernel), floored."""
    r64, r32 = _autograd(fn, inputs, dy, torch.float64), _autograd(fn, inputs, dy, torch.float32)
    return r64, [max(4 * _measure(b, a), floor) for a, b in zip(r64, r32)]


def _assert_within(request, names, gots, refs, lims):
    for name, got, ref, lim in zip(names, gots, refs, lims):
        err = _measure(got, ref)
        nm.note(request, f"{name}: max error / max |reference| {err:.3e}, {err / lim:.3f} of its limit {lim:.1e}")
        assert err <= lim, f"{name}: {err:.3e} > {lim:.3e}"


GN_BWD_SHAPE = (2, 64, 64, 32)      # n, hw, c0, c1: three channels per group, group 21 straddles the seam


def _gn_forward_on_device(ops, x, c0, c1, gamma, beta, n, hw, eps=1e-5):
    from dsml_thesis_amd import lib as L, train_ops as T
    x0d = x[..., :c0].contiguous().cuda()
    x1d = x[..., c0:].contiguous().cuda() if c1 else None
    chunks = L.load().ldmk_gn_chunks(hw)
    partial = torch.empty(n * chunks * (c0 + c1) * 3, device="cuda")
    coef = ops.gn_coef(x0d, x1d, n, hw, gamma.cuda(), beta.cuda(), eps, partial=partial)
    p1 = partial[n * chunks * c0 * 3:] if c1 else None
    return x0d, x1d, coef, T.gn_group_stats(partial, c0, p1, c1, n, hw, 32, eps)


@pytest.mark.parametrize("silu", [True, False])
def test_gn_bwd_on_mean_dominated_groups(ops, request, silu):
    from dsml_thesis_amd import train_ops as T
    n, hw, c0, c1 = GN_BWD_SHAPE
    Cc = c0 + c1
    x, dy = nm.gn_input(nm.GN_SEED, n, hw, Cc), rnd(550, n, hw, Cc)
    gamma, beta = nm.affine(nm.GN_SEED + 1, Cc)

    def fn(x_, g_, b_):
        z = F.group_norm(x_.permute(0, 2, 1), 32, g_, b_, 1e-5).permute(0, 2, 1)
        return F.silu(z) if silu else z
    (_, dx, dg, db), (_, *lims) = _limits(fn, (x, gamma, beta), dy, 5e-5)
    x0d, x1d, coef, mr = _gn_forward_on_device(ops, x, c0, c1, gamma, beta, n, hw)
    dx0, dx1, dgk, dbk = T.gn_bwd(x0d, x1d, dy.cuda(), coef, mr, gamma.cuda(), n, hw, silu=silu)
    _assert_within(request, ("dx", "dgamma", "dbeta"), (torch.cat([dx0, dx1], -1), dgk, dbk), (dx, dg, db), lims)


def test_gn_film_bwd_on_mean_dominated_groups(ops, request):
    from dsml_thesis_amd import train_ops as T
    n, hw, c0, c1 = GN_BWD_SHAPE
    Cc = c0 + c1                                               # (one source: the FiLM form takes no concat)
    x, dy = nm.gn_input(nm.GN_SEED, n, hw, Cc), rnd(550, n, hw, Cc)
    gamma, beta = nm.affine(nm.GN_SEED + 1, Cc)
    film = 0.3 * rnd(551, n, 2 * Cc)

    def fn(x_, g_, b_, f_):
        u = F.group_norm(x_.permute(0, 2, 1), 32, g_, b_, 1e-5).permute(0, 2, 1)
        return F.silu(u * (1 + f_[:, None, :Cc]) + f_[:, None, Cc:])
    (_, dx, dg, db, df), (_, *lims) = _limits(fn, (x, gamma, beta, film), dy, 5e-5)
    xd, _, coef, mr = _gn_forward_on_device(ops, x, Cc, 0, gamma, beta, n, hw)
    fd = film.cuda()
    T.gn_coef_film_(coef, fd)
    dfilm = torch.empty(n, 2 * Cc, device="cuda")
    dxk, dgk, dbk = T.gn_film_bwd(xd, dy.cuda(), coef, mr, gamma.cuda(), beta.cuda(), fd, n, hw, dfilm)
    _assert_within(request, ("dx", "dgamma", "dbeta", "dfilm"), (dxk, dgk, dbk, dfilm), (dx, dg, db, df), lims)


def test_ln_apply_and_ln_bwd_on_mean_dominated_rows(ops, request):
    from dsml_thesis_amd import train_ops as T
    rows, Cw = 33, 320
    x, dy = nm.ln_input(nm.LN_SEED, rows, Cw), rnd(552, rows, Cw)
    gamma, beta = nm.affine(nm.LN_SEED + 1, Cw)
    (y, dx, dg, db), lims = _limits(lambda x_, g_, b_: F.layer_norm(x_, (Cw,), g_, b_, 1e-5), (x, gamma, beta), dy, 3e-5)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    stats = ops.ln_stats(xd)
    yk = T.ln_apply(xd, stats, gd, bd)
    dxk, dgk, dbk = T.ln_bwd(dy.cuda(), xd, stats, gd)
    _assert_within(request, ("y", "dx", "dgamma", "dbeta"), (yk, dxk, dgk, dbk), (y, dx, dg, db), lims)
    # ... and the forward output element by element: the coefficient bound with the row in the place of the group, + 4 * 2^-24 |y|
    mean, rstd = nm.ln_ref(x)
    err = (yk.cpu().double() - y).abs()
    used = (err / nm.ln_out_bound(x, mean, rstd, gamma, y)).max().item()
    _report(request, "ln_apply per element", err.max().item(), used)
    assert used <= 1.0
