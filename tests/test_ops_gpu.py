"""GPU: every C-ABI kernel against the oracle / golden fixtures (per-op parity, fp32).

Tolerances: the HIP kernels accumulate in fp32 on the matrix cores in a different order than
PyTorch-CPU, so products over K terms differ by O(sqrt(K))*eps relative; stated per test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, rnd
from oracle import ldm_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu
T = lambda a: torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def ops():
    from dsml_thesis_amd import ops as ops_
    from dsml_thesis_amd import lib
    lib.load()
    return ops_


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(y):
    return y.permute(0, 3, 1, 2).contiguous().cpu()


def close(a, b, rtol=1e-4, atol=1e-4):
    torch.testing.assert_close(a.float().cpu(), torch.as_tensor(b).float().cpu(), rtol=rtol, atol=atol)


def test_version_and_error_path(ops):
    from dsml_thesis_amd import lib
    assert lib.load().ldmk_version() >= 100
    x = torch.zeros(4, 48, device="cuda")
    with pytest.raises(lib.LdmkError, match="multiples of 32"):
        ops.linear(x, torch.zeros(48, 32, device="cuda"))


@pytest.mark.parametrize("shape,c_split,eps", [((2, 160, 8, 8), None, 1e-5), ((1, 480, 4, 4), 320, 1e-5),
                                                ((3, 320, 16, 16), None, 1e-6), ((2, 960, 8, 8), 640, 1e-5),
                                                ((1, 128, 40, 24), None, 1e-6)])
def test_gn_coef(ops, shape, c_split, eps):
    n, c, h, w = shape
    x = rnd(1, *shape) * 1.5 + 0.3
    gamma, beta = 1 + 0.1 * rnd(2, c), 0.1 * rnd(3, c)
    xs = nhwc(x)
    if c_split:
        x0, x1 = xs[..., :c_split].contiguous(), xs[..., c_split:].contiguous()
    else:
        x0, x1 = xs, None
    coef = ops.gn_coef(x0, x1, n, h * w, gamma.cuda(), beta.cuda(), eps)
    y = xs * coef[:, 0].reshape(n, 1, 1, c) + coef[:, 1].reshape(n, 1, 1, c)
    close(nchw(y), F.group_norm(x, 32, gamma, beta, eps), 1e-5, 2e-5)


def test_gn_golden(ops):
    g = golden("g3_ops.npz")
    for tag, shape, seed in (("gn160", (2, 160, 8, 8), 11), ("gn480", (1, 480, 4, 4), 12)):
        sd = W.synth_state_dict({"weight": (shape[1],), "bias": (shape[1],)}, seed=1)
        x = rnd(seed, *shape) * 1.5 + 0.3
        xs = nhwc(x)
        coef = ops.gn_coef(xs, None, shape[0], shape[2] * shape[3], sd["weight"].cuda(), sd["bias"].cuda(), 1e-5)
        y = F.silu(xs * coef[:, 0].reshape(shape[0], 1, 1, -1) + coef[:, 1].reshape(shape[0], 1, 1, -1))
        close(nchw(y), g[tag], 1e-5, 2e-5)


@pytest.mark.parametrize("rows,c", [(300, 320), (65, 160), (7, 1024), (33, 150), (4096, 640)])
def test_ln_stats(ops, rows, c):
    x = (rnd(5, rows, c) * 2 + 0.5)
    st = ops.ln_stats(x.cuda()).cpu()
    close(st[:, 0], x.mean(1), 1e-5, 1e-5)
    close(st[:, 1], 1 / torch.sqrt(x.var(1, unbiased=False) + 1e-5), 1e-5, 1e-5)


CONV_CASES = [
    # n, cin, cout, h, w, stride, upsample, pad_lo
    (1, 160, 320, 8, 8, 1, False, 1),
    (2, 32, 64, 5, 7, 1, False, 1),        # ragged spatial size, partial tiles
    (2, 160, 160, 16, 16, 2, False, 1),    # Downsample
    (2, 160, 160, 8, 8, 1, True, 1),       # Upsample folded into the gather
    (1, 128, 128, 16, 16, 2, False, 0),    # VQGAN encoder asymmetric pad (0,1,0,1)
    (3, 640, 640, 8, 8, 1, False, 1),      # long K at low resolution (split-K path)
    (1, 64, 96, 32, 32, 1, False, 1),
]


@pytest.mark.parametrize("case", CONV_CASES)
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, 6])
def test_conv3x3(ops, case, cfg):
    from dsml_thesis_amd import lib
    n, cin, cout, h, w, stride, up, pad_lo = case
    x = rnd(10, n, cin, h, w)
    wt = rnd(11, cout, cin, 3, 3) / np.sqrt(9 * cin)
    b = 0.1 * rnd(12, cout)
    xi = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    if pad_lo == 0:
        ref = F.conv2d(F.pad(xi, (0, 1, 0, 1)), wt, b, stride=stride)
    else:
        ref = F.conv2d(xi, wt, b, stride=stride, padding=1)
    lib.load().ldmk_igemm_force_config(cfg)
    try:
        y = ops.conv3x3(nhwc(x), ops.pack_conv3x3(wt.cuda()), b.cuda(), stride=stride, pad_lo=pad_lo, upsample=up)
    finally:
        lib.load().ldmk_igemm_force_config(0)
    assert tuple(y.shape) == (n, ref.shape[2], ref.shape[3], cout)
    close(nchw(y), ref, 1e-4, 1e-4)


@pytest.mark.parametrize("splitk", [2, 3, 8])
def test_conv3x3_split_k_reduce(ops, splitk):
    n, cin, cout, h, w = 2, 640, 640, 8, 8
    x, wt, b = rnd(10, n, cin, h, w), rnd(11, cout, cin, 3, 3) / np.sqrt(9 * cin), 0.1 * rnd(12, cout)
    vec, res = rnd(13, n, cout), rnd(14, n, cout, h, w)
    ref = F.conv2d(x, wt, b, padding=1) + vec[:, :, None, None] + res
    ws = torch.empty(splitk * n * h * w * cout, device="cuda")
    out = torch.empty(n, h, w, cout, device="cuda")
    xd, wd, bd, vd, rd = nhwc(x), ops.pack_conv3x3(wt.cuda()), b.cuda(), vec.cuda(), nhwc(res)   # keep alive: raw pointers
    a = ops.make_igemm_args(n * h * w, cout, 9 * cin, xd, cin, wd, out, cout, h * w,
                            conv=(h, w, h, w, 1, 1, 0), bias=bd, batch_vec=vd, batch_vec_ld=cout,
                            residual=rd, splitk=splitk, splitk_ws=ws)
    ops.igemm(a)
    close(nchw(out), ref, 1e-4, 1e-4)
    out2 = torch.empty_like(out)
    a.out = out2.data_ptr()
    ops.igemm(a)
    assert torch.equal(out, out2), "split-K partials are summed in a fixed order"


@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("splitk", [2, 5, 16])
def test_split_k_in_launch_combine_equals_the_two_launch_form(ops, cfg, splitk):
    """One launch: each tile's last-arriving workgroup sums the slabs in the fixed order and runs the epilogue (bias,
    per-sample vector, residual, GroupNorm partial records).  Bitwise equal to main + reduce launches, launch after launch
    (the counters are left zeroed), for every workgroup tile shape incl. the ones that split K over their own waves."""
    n, cin, cout, h, w = 4, 320, 320, 16, 16
    x, wt, b = rnd(10, n, cin, h, w), rnd(11, cout, cin, 3, 3) / np.sqrt(9 * cin), 0.1 * rnd(12, cout)
    vec, res = rnd(13, n, cout), rnd(14, n, cout, h, w)
    xd, wd, bd, vd, rd = nhwc(x), ops.pack_conv3x3(wt.cuda()), b.cuda(), vec.cuda(), nhwc(res)
    ws = torch.empty(splitk * n * h * w * cout, device="cuda")
    cnt = torch.zeros(1024, device="cuda", dtype=torch.int32)
    outs, parts = [], []
    for counters in (None, cnt, cnt, cnt):
        out = torch.empty(n, h, w, cout, device="cuda")
        part = torch.zeros(n * h * w // 32, cout, 3, device="cuda")
        a = ops.make_igemm_args(n * h * w, cout, 9 * cin, xd, cin, wd, out, cout, h * w, conv=(h, w, h, w, 1, 1, 0), bias=bd,
                                batch_vec=vd, batch_vec_ld=cout, residual=rd, splitk=splitk, splitk_ws=ws, tile_cfg=cfg,
                                splitk_counters=counters)
        a.stats_out = part.data_ptr()
        ops.igemm(a)
        outs.append(out)
        parts.append(part)
    torch.cuda.synchronize()
    assert int(cnt.abs().sum()) == 0, "every launch must leave the arrival counters zeroed"
    ref = F.conv2d(x, wt, b, padding=1) + vec[:, :, None, None] + res
    close(nchw(outs[0]), ref, 1e-4, 1e-4)
    for o, p_ in zip(outs[1:], parts[1:]):
        assert torch.equal(o, outs[0]) and torch.equal(p_, parts[1])
    # the GroupNorm records of the two forms sum the same 32 values in a different order: same sums to fp32 accuracy
    full = lambda q: (q[..., 1] + 32 * q[..., 0], q[..., 2] + 2 * q[..., 0] * q[..., 1] + 32 * q[..., 0] ** 2)
    for u, v in zip(full(parts[1]), full(parts[0])):
        close(u, v, 1e-4, 1e-4)


def test_split_k_scratch_sized_from_the_abi_query_alone(ops):
    """A host that is not PyTorch: plan -> ldmk_igemm_workspace_elems -> allocate exactly that -> run."""
    import ctypes as C
    from dsml_thesis_amd import lib as L
    lib = L.load()
    assert lib.ldmk_init(torch.cuda.current_device()) == 0
    n, cin, cout, h, w = 2, 640, 640, 8, 8
    x, wt, b = rnd(10, n, cin, h, w), rnd(11, cout, cin, 3, 3) / np.sqrt(9 * cin), 0.1 * rnd(12, cout)
    xd, wd, bd = nhwc(x), ops.pack_conv3x3(wt.cuda()), b.cuda()
    out = torch.empty(n, h, w, cout, device="cuda")
    a = ops.make_igemm_args(n * h * w, cout, 9 * cin, xd, cin, wd, out, cout, h * w, conv=(h, w, h, w, 1, 1, 0), bias=bd)
    a.splitk_ws, a.splitk_ws_elems = 1, 1 << 40                 # "plan as if scratch were free"
    cfg, sk = C.c_int(0), C.c_int(0)
    assert lib.ldmk_igemm_plan(C.byref(a), C.byref(cfg), C.byref(sk)) == 0 and sk.value > 1
    a.tile_cfg, a.splitk, a.splitk_ws, a.splitk_ws_elems = cfg.value, sk.value, 0, 0
    need = lib.ldmk_igemm_workspace_elems(C.byref(a))
    assert need == sk.value * n * h * w * cout
    assert lib.ldmk_igemm(C.byref(a), ops.stream()) == -3       # LDMK_ENOMEM: no scratch given for the pinned plan
    ws = torch.empty(need, device="cuda")
    a.splitk_ws, a.splitk_ws_elems = ws.data_ptr(), need
    L.call("ldmk_igemm", C.byref(a), ops.stream())
    close(nchw(out), F.conv2d(x, wt, b, padding=1), 1e-4, 1e-4)


@pytest.mark.parametrize("splitk", [1, 4])
def test_igemm_emits_groupnorm_partials(ops, splitk):
    """The conv epilogue (and the split-K reduce) emit the same per-32-pixel-chunk records as ldmk_gn_partial, so the
    GroupNorm of the *output* needs no statistics pass."""
    from dsml_thesis_amd import lib as L
    n, cin, cout, h, w = 2, 160, 320, 8, 8
    x, wt, b = rnd(10, n, cin, h, w), rnd(11, cout, cin, 3, 3) / np.sqrt(9 * cin), 0.5 + 0.1 * rnd(12, cout)
    res = rnd(14, n, cout, h, w)
    xd, wd, bd, rd = nhwc(x), ops.pack_conv3x3(wt.cuda()), b.cuda(), nhwc(res)
    out = torch.empty(n, h, w, cout, device="cuda")
    part = torch.zeros(n * h * w // 32, cout, 3, device="cuda")
    ws = torch.empty(splitk * n * h * w * cout, device="cuda")
    a = ops.make_igemm_args(n * h * w, cout, 9 * cin, xd, cin, wd, out, cout, h * w, conv=(h, w, h, w, 1, 1, 0), bias=bd,
                            residual=rd, splitk=splitk, splitk_ws=ws)
    a.stats_out = part.data_ptr()
    ops.igemm(a)
    gamma, beta = 1 + 0.1 * rnd(21, cout), 0.1 * rnd(22, cout)
    gd, btd = gamma.cuda(), beta.cuda()                      # keep alive: the ABI takes raw pointers
    coef = torch.empty(n, 2, cout, device="cuda")
    L.call("ldmk_gn_finalize", part.data_ptr(), cout, 0, 0, n, h * w, 32, 1e-5, gd.data_ptr(), btd.data_ptr(),
           coef.data_ptr(), ops.stream())
    ref = F.group_norm(F.conv2d(x, wt, b, padding=1) + res, 32, gamma, beta, 1e-5)
    y = out * coef[:, 0].reshape(n, 1, 1, cout) + coef[:, 1].reshape(n, 1, 1, cout)
    close(nchw(y), ref, 1e-4, 1e-4)
    coef2 = ops.gn_coef(out, None, n, h * w, gd, btd, 1e-5)
    close(coef, coef2, 1e-5, 1e-5)


def test_gn_apply_concat(ops):
    n, c0, c1, h, w = 2, 320, 160, 8, 8
    x = rnd(20, n, c0 + c1, h, w) * 1.3 + 0.2
    gamma, beta = 1 + 0.1 * rnd(21, c0 + c1), 0.1 * rnd(22, c0 + c1)
    xs = nhwc(x)
    x0, x1 = xs[..., :c0].contiguous(), xs[..., c0:].contiguous()
    coef = ops.gn_coef(x0, x1, n, h * w, gamma.cuda(), beta.cuda(), 1e-5)
    y = ops.gn_apply(x0, x1, coef, n, h * w, silu=True).view(n, h, w, c0 + c1)
    close(nchw(y), F.silu(F.group_norm(x, 32, gamma, beta, 1e-5)), 1e-5, 2e-5)
    y = ops.gn_apply(x0, x1, coef, n, h * w, silu=False).view(n, h, w, c0 + c1)
    close(nchw(y), F.group_norm(x, 32, gamma, beta, 1e-5), 1e-5, 2e-5)


def test_conv3x3_golden_and_fused_prologue_epilogue(ops):
    g = golden("g3_ops.npz")
    sd = W.synth_state_dict({"weight": (320, 160, 3, 3), "bias": (320,)}, seed=2)
    y = ops.conv3x3(nhwc(rnd(13, 1, 160, 8, 8)), ops.pack_conv3x3(sd["weight"].cuda()), sd["bias"].cuda())
    close(nchw(y), g["conv3x3"], 1e-4, 1e-4)
    # GN+SiLU prologue over a concat of two tensors + per-sample vector + residual epilogue
    n, c0, c1, cout, h, w = 2, 320, 160, 320, 8, 8
    x = rnd(20, n, c0 + c1, h, w) * 1.3 + 0.2
    gamma, beta = 1 + 0.1 * rnd(21, c0 + c1), 0.1 * rnd(22, c0 + c1)
    wt, b = rnd(23, cout, c0 + c1, 3, 3) / np.sqrt(9 * (c0 + c1)), 0.1 * rnd(24, cout)
    vec, res = rnd(25, n, cout), rnd(26, n, cout, h, w)
    ref = F.conv2d(F.silu(F.group_norm(x, 32, gamma, beta, 1e-5)), wt, b, padding=1) + vec[:, :, None, None] + res
    xs = nhwc(x)
    x0, x1 = xs[..., :c0].contiguous(), xs[..., c0:].contiguous()
    coef = ops.gn_coef(x0, x1, n, h * w, gamma.cuda(), beta.cuda(), 1e-5)
    y = ops.conv3x3(x0, ops.pack_conv3x3(wt.cuda()), b.cuda(), x1=x1, coef=coef, silu=True, batch_vec=vec.cuda(),
                    residual=nhwc(res))
    close(nchw(y), ref, 1e-4, 2e-4)


@pytest.mark.parametrize("M,K,N", [(64, 160, 160), (1024, 640, 1920), (300, 320, 96), (4096, 160, 480)])
@pytest.mark.parametrize("b_trans", [False, True])
def test_linear_layernorm_prologue(ops, M, K, N, b_trans):
    x = rnd(30, M, K) * 1.2 + 0.1
    w, b = rnd(31, N, K) / np.sqrt(K), 0.1 * rnd(32, N)
    g, be = 1 + 0.1 * rnd(33, K), 0.1 * rnd(34, K)
    res = rnd(35, M, N)
    ref = F.linear(F.layer_norm(x, (K,), g, be, 1e-5), w, b) + res
    xc = x.cuda()
    st = ops.ln_stats(xc)
    wp = w.cuda() if b_trans else ops.pack_linear(w.cuda())
    y = ops.linear(xc, wp, b.cuda(), row_stats=st, ln_gamma=g.cuda(), ln_beta=be.cuda(), residual=res.cuda(),
                   b_trans=b_trans)
    close(y, ref, 1e-4, 1e-4)


ROW_TILES = {7: (1, 5), 8: (2, 5), 9: (1, 4), 10: (2, 4), 11: (1, 2), 12: (1, 1)}


@pytest.mark.parametrize("cfg", sorted(ROW_TILES))
@pytest.mark.parametrize("case", [
    # M, c0, c1, N, rows_per_sample, prologue, epilogue options
    (256, 160, 0, 160, 64, "none", "bias+vec+res+stats"),
    (300, 320, 0, 640, 300, "ln", "bias+res"),              # ragged M: clamped loads, masked stores
    (512, 160, 0, 1280, 128, "ln", "geglu"),
    (256, 320, 160, 320, 64, "none", "bias"),               # two-source channel concat (skip 1x1 conv)
    (512, 160, 0, 160, 128, "affine", "bias"),              # GroupNorm-affine prologue (proj_in)
    (64, 640, 0, 1920, 64, "ln", "none"),
])
def test_row_gemm_wave_tiles(ops, cfg, case):
    """The wave-autonomous row GEMM (csrc/rgemm.hip, tile_cfg 7..12) against torch fp32 and, bitwise, against itself."""
    M, c0, c1, N, rps, pro, epi = case
    tm, tn = ROW_TILES[cfg]
    fits = not (N % (32 * tn) or (epi == "geglu" and tn % 2) or (("vec" in epi or pro == "affine") and rps % (32 * tm)))
    K = c0 + c1
    x = rnd(70, M, K) * 1.2 + 0.1
    w, b = rnd(71, N, K) / np.sqrt(K), 0.1 * rnd(72, N)
    g, be = 1 + 0.1 * rnd(73, K), 0.1 * rnd(74, K)
    nsmp = (M + rps - 1) // rps
    vec, res = rnd(75, nsmp, N), rnd(76, M, N)
    sc, sh = 1 + 0.2 * rnd(77, nsmp, K), 0.3 * rnd(78, nsmp, K)
    a_ref = x
    if pro == "ln":
        a_ref = F.layer_norm(x, (K,), g, be, 1e-5)
    elif pro == "affine":
        a_ref = x * sc.repeat_interleave(rps, 0)[:M] + sh.repeat_interleave(rps, 0)[:M]
    y_ref = a_ref @ w.t()
    xc = x.cuda()
    x0 = xc[:, :c0].contiguous()
    x1 = xc[:, c0:].contiguous() if c1 else None
    kw = {}
    if pro == "ln":
        kw.update(row_stats=ops.ln_stats(xc), ln_gamma=g.cuda(), ln_beta=be.cuda())
    elif pro == "affine":
        kw.update(coef=torch.stack([sc, sh], 1).contiguous().cuda())
    part = None
    if epi == "geglu":
        wp, bp = ops.pack_geglu(w.cuda(), b.cuda())
        kw.update(geglu=True, bias=bp)
        v_, g_ = (y_ref + b).chunk(2, dim=1)
        y_ref = v_ * F.gelu(g_)
    else:
        wp = ops.pack_linear(w.cuda())
        if "bias" in epi:
            kw.update(bias=b.cuda())
            y_ref = y_ref + b
        if "vec" in epi:
            kw.update(batch_vec=vec.cuda())
            y_ref = y_ref + vec.repeat_interleave(rps, 0)[:M]
        if "res" in epi:
            kw.update(residual=res.cuda())
            y_ref = y_ref + res
        if "stats" in epi:
            part = torch.zeros(M // 32, N, 3, device="cuda")
            kw.update(stats_out=part)
    wf = ops.pack_wfrag(wp)
    if not fits:          # a wave tile that does not divide the problem is refused loudly, never run on a fallback
        from dsml_thesis_amd import lib as L
        with pytest.raises(L.LdmkError, match="row GEMM"):
            ops.linear(x0, wp, x1=x1, rows_per_sample=rps, w_frag=wf, tile_cfg=cfg, **kw)
        return
    y = ops.linear(x0, wp, x1=x1, rows_per_sample=rps, w_frag=wf, tile_cfg=cfg, **kw)
    close(y, y_ref, 1e-4, 1e-4)
    y2 = ops.linear(x0, wp, x1=x1, rows_per_sample=rps, w_frag=wf, tile_cfg=cfg, **kw)
    assert torch.equal(y, y2)
    if part is not None:      # the GroupNorm partial records of the output equal the stand-alone statistics pass
        ref_part = torch.empty_like(part)
        from dsml_thesis_amd import lib as L
        L.call("ldmk_gn_partial", y.data_ptr(), N, nsmp, rps, ref_part.data_ptr(), ops.stream())
        full = lambda p_: (p_[..., 1] + 32 * p_[..., 0], p_[..., 2] + 2 * p_[..., 0] * p_[..., 1] + 32 * p_[..., 0] ** 2)
        for u, v in zip(full(part), full(ref_part)):
            close(u, v, 1e-4, 1e-4)


@pytest.mark.parametrize("cfg,splitk", [(1, 1), (2, 1), (3, 1), (4, 1), (4, 3), (5, 1), (6, 2), (7, 1), (8, 1), (9, 1), (10, 1),
                                        (11, 1), (12, 1)])
@pytest.mark.parametrize("case", [(300, 320, 640, "res"), (512, 160, 1280, "geglu"), (64, 640, 1920, "none")])
def test_linear_layernorm_folded_through_the_product(ops, cfg, splitk, case):
    """LDMK_TF_LAYERNORM_FOLDED: LN(x) W + b computed as rstd (x W' - mean colsum(W')) + (beta^T W + b) with W' = diag(gamma) W
    (attention.py:203-205 followed by :161-168 / :37-64).  Rows carry a mean of the order of their spread, as the token
    rows of a transformer block do; the reference is float64, the tolerance the one of the unfolded prologue's test."""
    from dsml_thesis_amd import lib as L
    M, K, N, epi = case
    x = rnd(90, M, K) * 1.2 + 0.8 * rnd(91, M, 1) + 0.3
    w, b = rnd(92, N, K) / np.sqrt(K), 0.1 * rnd(93, N)
    g, be = 1 + 0.2 * rnd(94, K), 0.2 * rnd(95, K)
    res = rnd(96, M, N)
    ref = F.linear(F.layer_norm(x.double(), (K,), g.double(), be.double(), 1e-5), w.double(), b.double())
    xc = x.cuda()
    kw = dict(row_stats=ops.ln_stats(xc))
    if epi == "geglu":
        wp, bp = ops.pack_geglu(w.cuda(), b.cuda())
        v_, g_ = ref.chunk(2, dim=1)
        ref = v_ * F.gelu(g_)
        kw.update(geglu=True)
    else:
        wp, bp = ops.pack_linear(w.cuda()), b.cuda()
        if epi == "res":
            ref = ref + res.double()
            kw.update(residual=res.cuda())
    w2, cs, b2 = ops.fold_layernorm(wp, g.cuda(), be.cuda(), bp)
    close(w2, wp.cpu() * g[:, None], 0, 1e-7)
    close(cs, (wp.cpu().double() * g.double()[:, None]).sum(0).float(), 1e-5, 1e-5)
    wf = ops.pack_wfrag(w2) if cfg > 6 else None
    tn = ROW_TILES[cfg][1] if cfg > 6 else 1
    a = dict(ln_colsum=cs, w_frag=wf, tile_cfg=cfg, **kw)
    if cfg > 6 and (N % (32 * tn) or (epi == "geglu" and tn % 2)):
        with pytest.raises(L.LdmkError, match="row GEMM"):
            ops.linear(xc, w2, b2, **a)
        return
    if epi == "geglu" and (splitk > 1 or cfg in (5, 6)):
        return                      # GEGLU never splits K and runs on the even-column tiles (dispatch remaps the others)
    y = _linear_pinned(ops, xc, w2, b2, splitk, **a)
    close(y, ref.float(), 1e-4, 1e-4)
    # and it agrees with the unfolded prologue (same statistics, same weights) far inside that tolerance
    y3 = ops.linear(xc, wp, bp, ln_gamma=g.cuda(), ln_beta=be.cuda(), **kw)
    assert (y - y3).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
    with pytest.raises(L.LdmkError, match="folded layernorm"):
        ops.linear(xc, w2, b2, ln_colsum=cs, row_stats=kw["row_stats"], stats_out=torch.zeros(M // 32 + 1, N, 3, device="cuda"))


def test_layernorm_guard_flags_mean_dominated_rows(ops):
    """ldmk_ln_stats_guard: same statistics as ldmk_ln_stats, and the device flag goes up exactly when some row has
    |mean| * rstd above the limit (or NaN statistics); widths on the float4 path and on the scalar path."""
    from dsml_thesis_amd import lib as L
    for K in (160, 90):
        x = rnd(96, 64, K)
        x[17] += 3.0 * x[17].std()
        st_ref = ops.ln_stats(x.cuda())
        ratio = (st_ref[:, 0].abs() * st_ref[:, 1]).max().item()
        assert 2.5 < ratio < 3.6
        for limit, want in ((ratio * 1.05, 0), (ratio * 0.95, 1)):
            flag, st = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.empty(64, 2, device="cuda")
            L.call("ldmk_ln_stats_guard", x.cuda().data_ptr(), 64, K, 1e-5, st.data_ptr(), limit, flag.data_ptr(), ops.stream())
            assert torch.equal(st, st_ref) and flag.item() == want, (K, limit)
        xn = x.clone()
        xn[3, 5] = float("nan")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        L.call("ldmk_ln_stats_guard", xn.cuda().data_ptr(), 64, K, 1e-5, st.data_ptr(), 1e9, flag.data_ptr(), ops.stream())
        assert flag.item() == 1


@pytest.mark.parametrize("ratio", [1.0, 4.0, 8.0, 30.0, 100.0])
def test_layernorm_folded_error_growth_with_mean_dominated_rows(ops, ratio):
    """The folded form subtracts mean * colsum(W') from x W' in fp32: when a row's |mean| is `ratio` times its spread the two
    terms cancel and the error grows ~ ratio * sqrt(K) * eps relative to the output scale.  This pins the growth (what a
    checkpoint with mean-dominated token rows would see) next to the unfolded prologue, which does not have it --
    LDMK_LN_UNFOLDED=1 is the supported switch for such checkpoints."""
    M, K, N = 256, 640, 640
    x = rnd(90, M, K) + ratio * (1.0 + 0.1 * rnd(91, M, 1))
    w, b = rnd(92, N, K) / np.sqrt(K), 0.1 * rnd(93, N)
    g, be = 1 + 0.2 * rnd(94, K), 0.2 * rnd(95, K)
    ref = F.linear(F.layer_norm(x.double(), (K,), g.double(), be.double(), 1e-5), w.double(), b.double()).float()
    xc = x.cuda()
    st = ops.ln_stats(xc)
    wp, bp = ops.pack_linear(w.cuda()), b.cuda()
    w2, cs, b2 = ops.fold_layernorm(wp, g.cuda(), be.cuda(), bp)
    err_f = (ops.linear(xc, w2, b2, ln_colsum=cs, row_stats=st).cpu() - ref).abs().max().item()
    err_u = (ops.linear(xc, wp, bp, ln_gamma=g.cuda(), ln_beta=be.cuda(), row_stats=st).cpu() - ref).abs().max().item()
    print(f"|mean|/std = {ratio:5.0f}: folded max error {err_f:.2e}, unfolded {err_u:.2e} (outputs up to {ref.abs().max().item():.1f})")
    assert err_u < 1e-4                                        # the unfolded prologue normalises before it multiplies
    assert err_f < 1e-4 * max(1.0, ratio / 5.0)                # measured: see DESIGN section 5
    from dsml_thesis_amd.unet import LN_GUARD_RATIO
    if ratio <= LN_GUARD_RATIO:                                # below the guard's limit the folded form stays inside the UNet bound
        assert err_f < 3e-5, (ratio, err_f)


def _linear_pinned(ops, x, wp, bias, splitk, **kw):
    """ops.linear with the split-K factor pinned (ops.linear itself leaves it to the plan)."""
    if splitk == 1:
        return ops.linear(x, wp, bias, **kw)
    from dsml_thesis_amd import lib as L
    M, K = x.shape
    N = wp.shape[1]
    out = torch.empty(M, N, device="cuda")
    a = ops.make_igemm_args(M, N, K, x, K, wp, out, N, M, tf=L.TF_LAYERNORM_FOLDED, row_stats=kw["row_stats"], bias=bias,
                            residual=kw.get("residual"), ln_colsum=kw["ln_colsum"], tile_cfg=kw["tile_cfg"], splitk=splitk)
    ws = torch.empty(splitk * M * N, device="cuda")
    a.splitk_ws, a.splitk_ws_elems = ws.data_ptr(), ws.numel()
    ops.igemm(a)
    return out


WINOGRAD_CASES = [
    # n, h, w, c0, c1, cout, GroupNorm+SiLU prologue, epilogue options
    (2, 16, 16, 64, 0, 96, True, "bias+vec+res+stats"),
    (1, 8, 8, 32, 32, 64, True, "bias+stats"),                 # channel concat; W = 8: two tile rows per GroupNorm chunk
    (3, 4, 32, 32, 0, 32, False, "bias+res"),                   # non-square, no prologue
    (1, 64, 64, 32, 0, 32, True, "bias+stats"),                 # W = 64: two chunks per image row
    (1, 4, 128, 32, 0, 32, True, "bias+stats"),                 # W = 128: eight chunks per band
]


def winograd_case(ops, case):
    """One case of WINOGRAD_CASES through ops.conv3x3_winograd: (result, its GroupNorm records or None, float64 reference)."""
    n, h, w, c0, c1, cout, pro, epi = case
    C_ = c0 + c1
    x = rnd(110, n, C_, h, w) * 1.3 + 0.2
    wt, b = rnd(111, cout, C_, 3, 3) / np.sqrt(9 * C_), 0.1 * rnd(112, cout)
    gamma, beta = 1 + 0.1 * rnd(113, C_), 0.1 * rnd(114, C_)
    vec, res = rnd(115, n, cout), rnd(116, n, cout, h, w)
    a = x.double()
    if pro:
        a = F.silu(F.group_norm(a, 32 if C_ % 32 == 0 else 8, gamma.double(), beta.double(), 1e-5))
    ref = F.conv2d(a, wt.double(), b.double(), padding=1)
    kw = dict(bias=b.cuda())
    if "vec" in epi:
        ref = ref + vec.double()[:, :, None, None]
        kw.update(batch_vec=vec.cuda())
    if "res" in epi:
        ref = ref + res.double()
        kw.update(residual=nhwc(res))
    xc = nhwc(x)
    x0 = xc[..., :c0].contiguous()
    x1 = xc[..., c0:].contiguous() if c1 else None
    if pro:
        kw.update(coef=ops.gn_coef(x0, x1, n, h * w, gamma.cuda(), beta.cuda(), 1e-5, groups=32 if C_ % 32 == 0 else 8))
    part = torch.zeros(n * h * w // 32, cout, 3, device="cuda") if "stats" in epi else None
    y = ops.conv3x3_winograd(x0, ops.pack_winograd(wt.cuda()), x1=x1, stats_out=part, **kw)
    return y, part, ref


@pytest.mark.parametrize("case", WINOGRAD_CASES)
def test_conv3x3_winograd_matches_conv2d(ops, case):
    """Winograd F(2x2,3x3) (csrc/winograd.hip + batched igemm) against F.conv2d in float64: openaimodel.py:201-204 / :226-230
    (GroupNorm -> SiLU -> Conv2d 3x3, + timestep vector, + skip).  Same tolerance as the direct implicit-GEMM convolution."""
    n, h, w, c0, c1, cout, pro, epi = case
    y, part, ref = winograd_case(ops, case)
    close(nchw(y), ref.float(), 1e-4, 1e-4)
    if part is not None:      # the GroupNorm partial records of the result equal the stand-alone statistics pass
        from dsml_thesis_amd import lib as L
        ref_part = torch.empty_like(part)
        L.call("ldmk_gn_partial", y.data_ptr(), cout, n, h * w, ref_part.data_ptr(), ops.stream())
        full = lambda p_: (p_[..., 1] + 32 * p_[..., 0], p_[..., 2] + 2 * p_[..., 0] * p_[..., 1] + 32 * p_[..., 0] ** 2)
        for got, want in zip(full(part.double()), full(ref_part.double())):
            close(got, want, 1e-4, 1e-3)


@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 8, 8, 64, 96), (1, 16, 32, 32, 32), (3, 4, 8, 32, 64), (1, 2, 64, 32, 32)])
def test_upsample_conv_phases_match_interpolate_conv2d(ops, n, h, w, cin, cout):
    """Upsample (nearest x2) + Conv2d 3x3 (openaimodel.py:107-118) as four 2x2-tap phase convolutions on the low-resolution
    input, against F.interpolate + F.conv2d in float64, and against the folded-gather implicit GEMM it replaces."""
    x = rnd(120, n, cin, h, w)
    wt, b = rnd(121, cout, cin, 3, 3) / np.sqrt(9 * cin), 0.1 * rnd(122, cout)
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), wt.double(), b.double(), padding=1)
    part = torch.zeros(n * 4 * h * w // 32, cout, 3, device="cuda")
    y = ops.upsample_conv3x3_phases(nhwc(x), ops.pack_upconv(wt.cuda()), b.cuda(), stats_out=part)
    close(nchw(y), ref.float(), 1e-4, 1e-4)
    y_direct = ops.conv3x3(nhwc(x), ops.pack_conv3x3(wt.cuda()), b.cuda(), upsample=True)
    close(y, y_direct, 1e-4, 1e-4)
    from dsml_thesis_amd import lib as L
    ref_part = torch.empty_like(part)
    L.call("ldmk_gn_partial", y.data_ptr(), cout, n, 4 * h * w, ref_part.data_ptr(), ops.stream())
    full = lambda p_: (p_[..., 1] + 32 * p_[..., 0], p_[..., 2] + 2 * p_[..., 0] * p_[..., 1] + 32 * p_[..., 0] ** 2)
    for got, want in zip(full(part.double()), full(ref_part.double())):
        close(got, want, 1e-4, 1e-3)


def test_row_gemm_rejects_what_it_cannot_run(ops):
    from dsml_thesis_amd import lib as L
    x, w = rnd(80, 64, 160).cuda(), rnd(81, 96, 160).cuda()
    wp = ops.pack_linear(w)
    with pytest.raises(L.LdmkError, match="w_frag"):
        ops.linear(x, wp, tile_cfg=7)                                   # no fragment copy given
    with pytest.raises(L.LdmkError, match="multiple of the tile"):
        ops.linear(x, wp, w_frag=ops.pack_wfrag(wp), tile_cfg=7)        # N = 96 is not a multiple of 160
    y = ops.linear(x, wp, w_frag=ops.pack_wfrag(wp), tile_cfg=12)       # 32-column tiles fit
    close(y, x.cpu() @ w.cpu().t(), 1e-4, 1e-4)


def test_geglu_ff_golden(ops):
    g = golden("g3_ops.npz")
    ff = {"net.0.proj.weight": (1280, 160), "net.0.proj.bias": (1280,), "net.2.weight": (160, 640), "net.2.bias": (160,)}
    sd = W.synth_state_dict(ff, seed=6)
    x = rnd(16, 1, 64, 160)[0].cuda()
    wp, bp = ops.pack_geglu(sd["net.0.proj.weight"].cuda(), sd["net.0.proj.bias"].cuda())
    h = ops.linear(x, wp, bp, geglu=True)
    y = ops.linear(h, ops.pack_linear(sd["net.2.weight"].cuda()), sd["net.2.bias"].cuda())
    close(y, g["geglu_ff"][0], 1e-4, 1e-4)


@pytest.mark.parametrize("n,tokens,heads", [(1, 64, 5), (2, 256, 10), (2, 1024, 5), (1, 4096, 5), (3, 96, 2),
                                            (2, 16, 3), (1, 77, 2), (1, 130, 1)])
@pytest.mark.parametrize("qt", [1, 2])
def test_attn_self(ops, n, tokens, heads, qt):
    from dsml_thesis_amd import lib
    lib.load().ldmk_attn_force_qt(qt)
    C = heads * 32
    qkv = rnd(40, n * tokens, 3 * C)
    qkv[:, :2 * C] *= 2.0         # make the softmax peaky enough to exercise the running-max rescale
    q, k, v = qkv.view(n, tokens, 3, heads, 32).permute(2, 0, 3, 1, 4).double()
    p = torch.softmax(q @ k.transpose(-1, -2) * 32 ** -0.5, dim=-1)
    ref = (p @ v).permute(0, 2, 1, 3).reshape(n * tokens, C).float()
    try:
        y = ops.attn_self(qkv.cuda(), n, tokens, heads)
    finally:
        lib.load().ldmk_attn_force_qt(0)
    close(y, ref, 1e-4, 2e-5)


def test_attn_self_rescale_branch(ops):
    # one key spikes late in the sequence -> running max jumps on the last tile (online-softmax rescale)
    n, tokens, heads, C = 1, 256, 1, 32
    qkv = rnd(41, tokens, 3 * C) * 0.1
    qkv[200, C:2 * C] = qkv[7, :C] * 400.0
    q, k, v = qkv.view(1, tokens, 3, 1, 32).permute(2, 0, 3, 1, 4).double()
    ref = (torch.softmax(q @ k.transpose(-1, -2) * 32 ** -0.5, -1) @ v).permute(0, 2, 1, 3).reshape(tokens, C).float()
    close(ops.attn_self(qkv.cuda(), n, tokens, heads), ref, 1e-4, 2e-5)


def test_attention_golden(ops):
    g = golden("g3_ops.npz")
    x = rnd(16, 1, 64, 160)[0].cuda()
    ca = {"to_q.weight": (160, 160), "to_k.weight": (160, 160), "to_v.weight": (160, 160),
          "to_out.0.weight": (160, 160), "to_out.0.bias": (160,)}
    sd = W.synth_state_dict(ca, seed=4)
    wqkv = torch.cat([sd["to_q.weight"], sd["to_k.weight"], sd["to_v.weight"]], 0).cuda()
    qkv = ops.linear(x, ops.pack_linear(wqkv))
    o = ops.attn_self(qkv, 1, 64, 5)
    y = ops.linear(o, ops.pack_linear(sd["to_out.0.weight"].cuda()), sd["to_out.0.bias"].cuda())
    close(y, g["attn_self"][0], 1e-4, 1e-4)
    ca["to_k.weight"] = ca["to_v.weight"] = (160, 512)
    sd = W.synth_state_dict(ca, seed=5)
    q = ops.linear(x, ops.pack_linear(sd["to_q.weight"].cuda()))
    for Lc in (1, 3):
        ctx = rnd(17 + Lc, 1, Lc, 512)[0].cuda()
        k = ops.dense_small(ctx, ops.pack_linear(sd["to_k.weight"].cuda()))
        v = ops.dense_small(ctx, ops.pack_linear(sd["to_v.weight"].cuda()))
        o = ops.attn_cross(q, k, v, 1, 64, Lc, 5)
        y = ops.linear(o, ops.pack_linear(sd["to_out.0.weight"].cuda()), sd["to_out.0.bias"].cuda())
        close(y, g[f"attn_cross_L{Lc}"][0], 1e-4, 1e-4)


def test_dense_small_and_timestep_embedding(ops):
    g = golden("g2_timestep_embedding.npz")
    t = T(g["t"]).cuda()
    emb = ops.timestep_embedding(t, ops.timestep_freqs(160), 160)
    # the angle t*freq reaches ~1e3 rad, where 1 ulp of the fp32 frequency table (host expf differs by an
    # ulp between CPUs / SIMD paths -- the reference itself is not bit-stable across hosts here) moves
    # sin/cos by up to 6e-5; everything else in the kernel is exact to fp32 rounding
    close(emb, g["emb"], 0, 1.3e-4)
    close(emb[:2], g["emb"][:2], 0, 1e-6)       # t in {0, 1}: small angles, tight
    x, w, b = rnd(50, 19, 640), rnd(51, 1000, 640) / 25.0, rnd(52, 1000)
    y = ops.dense_small(x.cuda(), ops.pack_linear(w.cuda()), b.cuda(), silu_in=True)
    close(y, F.linear(F.silu(x), w, b), 1e-4, 1e-4)


def test_boundary_convs(ops):
    x0, x1 = rnd(60, 2, 3, 12, 10), rnd(61, 2, 6, 12, 10)
    w, b = rnd(62, 160, 9, 3, 3) / 9.0, rnd(63, 160)
    y = ops.conv3x3_in(x0.cuda(), ops.pack_conv3x3_narrow(w.cuda()), b.cuda(), 160, x1=x1.cuda())
    close(nchw(y), F.conv2d(torch.cat([x0, x1], 1), w, b, padding=1), 1e-5, 1e-5)
    x = rnd(64, 2, 160, 9, 11) * 1.4
    gamma, beta = 1 + 0.1 * rnd(65, 160), 0.1 * rnd(66, 160)
    w, b = rnd(67, 3, 160, 3, 3) / 38.0, rnd(68, 3)
    xs = nhwc(x)
    coef = ops.gn_coef(xs, None, 2, 99, gamma.cuda(), beta.cuda(), 1e-5)
    y = ops.conv3x3_out(xs, coef, ops.pack_conv3x3_narrow(w.cuda()), b.cuda(), 3)
    close(y, F.conv2d(F.silu(F.group_norm(x, 32, gamma, beta, 1e-5)), w, b, padding=1), 1e-4, 1e-4)
    x, w, b = rnd(69, 2, 3, 8, 8), rnd(70, 3, 3, 1, 1), rnd(71, 3)
    close(ops.conv1x1_nchw(x.cuda(), w.cuda(), b.cuda()), F.conv2d(x, w, b), 1e-6, 1e-6)


@pytest.mark.parametrize("n,cin,cout,h,w", [(2, 4, 160, 64, 64), (1, 3, 512, 32, 32), (3, 9, 160, 5, 70), (1, 16, 96, 3, 130),
                                            (1, 1, 300, 7, 1)])
def test_conv3x3_in_row_segments(ops, n, cin, cout, h, w):
    """Row-segment kernel: widths below / at / above one 64-pixel segment, cout beyond one pass of 256 threads."""
    x, wt, b = rnd(160, n, cin, h, w), rnd(161, cout, cin, 3, 3) / 3.0, rnd(162, cout)
    y = ops.conv3x3_in(x.cuda(), ops.pack_conv3x3_narrow(wt.cuda()), b.cuda(), cout)
    close(nchw(y), F.conv2d(x, wt, b, padding=1), 1e-5, 2e-5)


@pytest.mark.parametrize("n,cin,cout,h,w,norm", [(2, 160, 4, 64, 64, True), (1, 128, 3, 48, 80, True), (2, 512, 4, 5, 19, True),
                                                 (1, 36, 1, 17, 16, False), (1, 160, 2, 1, 1, True)])
def test_conv3x3_out_tiles(ops, n, cin, cout, h, w, norm):
    """16x16-pixel tiles with a halo, 32-channel chunks (cin not a multiple of 32 too), ragged tiles, no-norm path."""
    x = rnd(170, n, cin, h, w) * 1.4
    wt, b = rnd(171, cout, cin, 3, 3) / np.sqrt(9 * cin), rnd(172, cout)
    xs = nhwc(x)
    coef, ref_in = None, x
    if norm:
        gamma, beta = 1 + 0.1 * rnd(173, cin), 0.1 * rnd(174, cin)
        coef = ops.gn_coef(xs, None, n, h * w, gamma.cuda(), beta.cuda(), 1e-5)
        ref_in = F.silu(F.group_norm(x, 32, gamma, beta, 1e-5))
    y = ops.conv3x3_out(xs, coef, ops.pack_conv3x3_narrow(wt.cuda()), b.cuda(), cout)
    close(y, F.conv2d(ref_in, wt, b, padding=1), 1e-4, 1e-4)


def test_sampler_updates_golden(ops):
    from dsml_thesis_amd import lib as L
    g = golden("g3_ops.npz")
    s = O.register_schedule(**W.SCHEDULE)
    ts = O.make_ddim_timesteps(200)
    tab = O.make_ddim_tables(s["alphas_cumprod"], ts, 1.0)
    table = torch.from_numpy(np.stack([tab["a_t"], tab["a_prev"], tab["sigma_t"], tab["sqrt_one_minus_at"]], 1)).cuda()
    x, e = rnd(31, 2, 3, 32, 32).cuda(), rnd(32, 2, 3, 32, 32).cuda()
    noise = T(g["ddim_noise"]).cuda()
    step = torch.tensor([100], dtype=torch.int32, device="cuda")
    tsd = torch.from_numpy(ts.astype(np.int64)).cuda()
    tcur = torch.zeros(2, dtype=torch.int64, device="cuda")
    xp, p0 = torch.empty_like(x), torch.empty_like(x)
    L.call("ldmk_ddim_step", x.data_ptr(), e.data_ptr(), noise.data_ptr(), table.data_ptr(), step.data_ptr(), 1.0, 0,
           xp.data_ptr(), p0.data_ptr(), 3 * 32 * 32, 2, tsd.data_ptr(), tcur.data_ptr(), 2, 1, 200, ops.stream())
    close(xp, g["ddim_x_prev"], 1e-6, 2e-6)
    close(p0, g["ddim_pred_x0"], 1e-6, 4e-6)
    assert step.item() == 99 and tcur.tolist() == [int(ts[99])] * 2
    # CFG combine inside the update: eps = [uncond | cond]
    e2 = torch.cat([rnd(33, 2, 3, 32, 32).cuda(), e])
    L.call("ldmk_ddim_step", x.data_ptr(), e2.data_ptr(), 0, table.data_ptr(), step.data_ptr(), 3.0, 1,
           xp.data_ptr(), p0.data_ptr(), 3 * 32 * 32, 2, 0, 0, 0, 0, 0, ops.stream())
    ec = O.cfg_combine(e2[:2].cpu(), e2[2:].cpu(), 3.0)
    rx, _ = O.ddim_update(x.cpu(), ec, tab["a_t"][99], tab["a_prev"][99], 0.0, tab["sqrt_one_minus_at"][99])
    # sigma from the eta=1 table still multiplies zero noise: compare against eta-1 coefficients, no noise
    rx, _ = O.ddim_update(x.cpu(), ec, tab["a_t"][99], tab["a_prev"][99], tab["sigma_t"][99],
                          tab["sqrt_one_minus_at"][99], torch.zeros(2, 3, 32, 32))
    close(xp, rx, 1e-6, 2e-6)
    # ancestral update
    tables = torch.stack([s["sqrt_recip_alphas_cumprod"], s["sqrt_recipm1_alphas_cumprod"], s["posterior_mean_coef1"],
                          s["posterior_mean_coef2"]], 1).contiguous().cuda()
    t = torch.tensor([0, 700], device="cuda")
    nz = T(g["ddpm_noise"]).cuda()
    L.call("ldmk_ddpm_step", x.data_ptr(), e.data_ptr(), nz.data_ptr(), tables.data_ptr(),
           s["posterior_log_variance_clipped"].cuda().data_ptr(), t.data_ptr(), xp.data_ptr(), 3 * 32 * 32, 2,
           ops.stream())
    close(xp, g["ddpm_x_prev"], 1e-6, 2e-6)


def test_vq_nearest_golden(ops):
    """Index work is bit-exact: the kernel restates the reference's fp32 rounding sequence (quantize.py:276-285)."""
    g = golden("g6_vqgan.npz")
    cb = W.synth_tensor("quantize.embedding.weight", (16384, 3))
    z = rnd(61, 1, 3, 32, 32)
    zq, idx = ops.vq_nearest(z.cuda(), torch.from_numpy(cb).cuda())
    assert np.array_equal(idx.cpu().numpy(), g["vq_idx"].reshape(-1))
    close(zq, g["vq_zq"], 0, 0)
    # dim-4 / 16384 codes on 4096 vectors: the north-star first stage (reference output, g11)
    g11 = golden("g11_northstar.npz")
    cb4 = torch.from_numpy(W.synth_tensor("quantize.embedding.weight", (16384, 4)))
    z4 = rnd(112, 1, 4, 64, 64)
    zq4, idx4 = ops.vq_nearest(z4.cuda(), cb4.cuda())
    assert np.array_equal(idx4.cpu().numpy(), g11["vq4_idx"].reshape(-1))
    close(zq4, g11["vq4_zq"], 0, 0)
    # small codebooks (fewer codes than lanes), ragged code counts, batch > 1: vs the oracle, all indices equal
    for seed, (n, dim, hw, ncode) in enumerate([(2, 4, 64, 512), (3, 3, 35, 37), (1, 4, 5, 1), (2, 3, 16, 100)]):
        zz = rnd(200 + seed, n, dim, hw, 1)
        cc = rnd(300 + seed, ncode, dim)
        q, i = ops.vq_nearest(zz.cuda(), cc.cuda())
        rq, ri = O.vq_quantize(zz, cc)
        assert torch.equal(i.cpu().long(), ri.reshape(-1))
        close(q, rq, 0, 0)


def test_vq_nearest_nan_rows_do_not_fault(ops):
    """A diverged latent (NaN) must give a valid index (torch.argmin: the first NaN -> 0), never an out-of-range gather."""
    cb = rnd(310, 1000, 3)
    z = rnd(311, 1, 3, 8, 8)
    z[0, 1, 2, 3] = float("nan")
    zq, idx = ops.vq_nearest(z.cuda(), cb.cuda())
    torch.cuda.synchronize()
    _, ri = O.vq_quantize(z, cb)
    assert torch.equal(idx.cpu().long(), ri.reshape(-1))
    assert int(idx.min()) >= 0 and int(idx.max()) < 1000


def test_bmm_softmax_postprocess(ops):
    a, b = rnd(80, 2, 96, 64), rnd(81, 2, 128, 64)
    s = ops.bmm(a.cuda(), b.cuda(), b_trans=True)
    close(s, a @ b.transpose(1, 2), 1e-4, 1e-4)
    ops.softmax_rows_(s.view(-1, 128), 0.125)
    close(s, torch.softmax((a @ b.transpose(1, 2)) * 0.125, -1), 1e-4, 1e-5)
    v = rnd(82, 2, 128, 32)
    close(ops.bmm(s, v.cuda(), b_trans=False), torch.softmax((a @ b.transpose(1, 2)) * 0.125, -1) @ v, 1e-4, 1e-4)
    x = rnd(83, 2, 3, 16, 16)
    close(ops.postprocess_frames(x.cuda()), O.postprocess_frames(x), 0, 1e-7)
    y = rnd(84, 128, 64).cuda()
    vec = rnd(85, 2, 64).cuda()
    ref = y.cpu() + vec.cpu().repeat_interleave(64, 0)
    close(ops.add_rowvec_(y, vec, 64), ref, 0, 1e-7)
