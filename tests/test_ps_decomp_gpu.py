"""GPU: the whole-round GEGLU tiles and the K groups inside the workgroup of the pre-split GEMM (csrc/igemm_ps.hip).

tile_cfg 34 / 35 (256x320 / 128x320, 32x320 wave tiles, F16X2 planes) are new instantiations of the kernel tile_cfg 28 runs: same K
order, so the same bits.  tile_cfg 40 / 48 (= 27 / 35 with two K groups, 36 + the base's index) give each group the K slice that
splitk = 2 gives a workgroup and form acc0 + acc1 inside the workgroup: the bits of the base tile at splitk = 2 plus the reduce
launch, for every epilogue -- also those the split over workgroups refuses (GEGLU, out_ps, attn_kv_out), which are held to a
float64 reference under the bounds tests/test_f16x2_gpu.py states for them.

Every output lives inside a larger buffer whose surroundings hold a sentinel: a write outside out, out_ps, the records, the
split-K slabs or the K / V tiles fails the test.  Every case is launched three times and must give identical bytes.

One case cannot be launched as written down for it: at K = 32 the second slice is empty, and the library refuses splitk = 2 there
("more K slices than 32-deep chunks").  Its reference is the base tile at splitk = 2 on the same problem with 32 columns of
zeros appended to A (and 32 rows of zeros to W): slice 0 is the K = 32 product, slice 1 sums exact zeros, and the reduce launch
forms 0 + s0 + 0 and writes the GroupNorm records in its own order -- the launch an empty second slice stands for.  With two A
sources K = 32 has no seam to put anywhere (both widths are positive multiples of 32): that variant runs at K = 96 only.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rnd
from test_ops_gpu import ops  # noqa: F401  (the `ops` fixture)

pytestmark = pytest.mark.gpu

GUARD = 4096            # sentinel elements on either side of every output
S32 = -7.0e30           # fp32 sentinel; 0xA5 for bytes


def padded(shape, dtype=torch.float32, fill=None):
    """(tensor of `shape` inside a sentinel-filled buffer, check()): check fails when anything outside the tensor was written"""
    n = int(np.prod(shape))
    sent = S32 if dtype == torch.float32 else 0xA5
    buf = torch.full((n + 2 * GUARD,), sent, dtype=dtype, device="cuda")
    view = buf[GUARD:GUARD + n].view(*shape)
    view.fill_(fill if fill is not None else (3.0 if dtype == torch.float32 else 0x3C))

    def check():
        assert bool((buf[:GUARD] == sent).all()) and bool((buf[GUARD + n:] == sent).all()), f"write outside a {tuple(shape)} output"
    return view, check


def padded_ps(ops, rows, k, h2):
    return padded((ops.ps_empty(rows, k, h2=h2).numel(),), torch.uint8)


def run3(make):
    """three launches into fresh buffers: identical bytes; returns the first run's outputs"""
    runs = []
    for _ in range(3):
        o = make()
        torch.cuda.synchronize()
        runs.append(o)
    for o in runs[1:]:
        for k in runs[0]:
            assert torch.equal(o[k], runs[0][k]), f"{k}: two launches of the same case differ"
    return runs[0]


def same(got, ref, what):
    for k in ref:
        d = (got[k].double() - ref[k].double()).abs().max().item() if got[k].dtype == torch.float32 else float((got[k] != ref[k]).sum().item())
        print(f"  {what} {k}: largest difference {d:.3e}")
    for k in ref:
        assert torch.equal(got[k], ref[k]), f"{what}: {k} is not bitwise the reference's"


def err(y, ref):
    d = y.detach().cpu().double() - ref
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


def f16x2_class(e32, eh, floor, what):
    """the bound of tests/test_f16x2_gpu.py (_f16x2_class): RMS error within 2x, worst element within 3x of the fp32 matrix-core form"""
    print(f"  {what}: (max, rms) error against float64: fp32 form {e32[0]:.3e} {e32[1]:.3e}, this tile {eh[0]:.3e} {eh[1]:.3e}")
    assert eh[1] <= max(2.0 * e32[1], 0.3 * floor), (e32, eh)
    assert eh[0] <= max(3.0 * e32[0], floor), (e32, eh)


def flag_():
    return torch.zeros(1, device="cuda", dtype=torch.int32)


# ------------------------------------------------------------------------------------------ problems
def rows_problem(ops, M, N, K, h2, seed, k0=0):
    x, w = rnd(seed, M, K).cuda(), (rnd(seed + 1, N, K) / np.sqrt(K)).cuda()
    wp = ops.pack_linear(w)
    flag = flag_()
    pk = lambda t: ops.pack_ps(t.contiguous(), h2_flag=flag if h2 else None)      # noqa: E731
    p = dict(M=M, N=N, K=K, x=x, w=w, wp=wp, wps=ops.pack_wps(wp, h2=h2), flag=flag, k0=k0, bias=(0.1 * rnd(seed + 2, N)).cuda(),
             res=rnd(seed + 3, M, N).cuda(), vec=rnd(seed + 4, (M + 31) // 32, N).cuda())
    p["a_ps"], p["a_ps1"] = (pk(x[:, :k0]), pk(x[:, k0:])) if k0 else (pk(x), None)
    return p


def launch_rows(ops, p, cfg, sk, form):
    """form "tr": bias + residual (transposed epilogue); "col": bias + per-sample vector + residual + GroupNorm records (lane = column)"""
    M, N, K = p["M"], p["N"], p["K"]
    checks = []
    out, c = padded((M, N))
    checks.append(c)
    kw = dict(tile_cfg=cfg, splitk=sk, a_ps=p["a_ps"], w_ps=p["wps"], range_flag=p["flag"], bias=p["bias"], residual=p["res"])
    if p["a_ps1"] is not None:
        kw.update(a_ps1=p["a_ps1"], a_ps_k0=p["k0"])
    if sk > 1:
        ws, c = padded((sk * M * N,))
        checks.append(c)
        kw["splitk_ws"] = ws
    rps = M
    if form == "col":
        kw.update(batch_vec=p["vec"], batch_vec_ld=N)
        rps = 32
    a = ops.make_igemm_args(M, N, K, None, K, p["wp"], out, N, rps, **kw)
    res = dict(out=out)
    if form == "col":
        rec, c = padded((M // 32, N, 3))
        checks.append(c)
        a.stats_out = rec.data_ptr()
        res["records"] = rec
    ops.igemm(a)
    torch.cuda.synchronize()
    for c in checks:
        c()
    assert int(p["flag"].item()) == 0
    return res


def geglu_problem(ops, M, N, K, seed):
    x = rnd(seed, M, K) + 0.5 * rnd(seed + 1, M, 1)
    w, b = rnd(seed + 2, N, K) / np.sqrt(K), 0.1 * rnd(seed + 3, N)
    g, be = 1 + 0.2 * rnd(seed + 4, K), 0.2 * rnd(seed + 5, K)
    wp, bp = ops.pack_geglu(w.cuda(), b.cuda())
    w2, cs, b2 = ops.fold_layernorm(wp, g.cuda(), be.cuda(), bp)
    flag = flag_()
    st, xps = ops.ln_stats_ps(x.cuda(), h2_flag=flag)
    return dict(M=M, N=N, K=K, x=x, w=w, b=b, g=g, be=be, w2=w2, cs=cs, b2=b2, st=st, xps=xps, wps=ops.pack_wps(w2, h2=True), flag=flag)


def launch_geglu(ops, p, cfg, with_fp32=True):
    from dsml_thesis_amd import lib as L
    M, N, K = p["M"], p["N"], p["K"]
    out, c0 = padded((M, N // 2))
    o_ps, c1 = padded_ps(ops, M, N // 2, True)
    a = ops.make_igemm_args(M, N, K, None, K, p["w2"], out if with_fp32 else None, N // 2, M, tf=L.TF_LAYERNORM_FOLDED, row_stats=p["st"],
                            ln_colsum=p["cs"], bias=p["b2"], epi=L.EPI_GEGLU, tile_cfg=cfg, splitk=1, a_ps=p["xps"], w_ps=p["wps"], out_ps=o_ps,
                            range_flag=p["flag"])
    ops.igemm(a)
    torch.cuda.synchronize()
    c0()
    c1()
    assert int(p["flag"].item()) == 0
    return dict(out=out, out_ps=o_ps) if with_fp32 else dict(out_ps=o_ps)


# ------------------------------------------------------------------------------------------ 1. the 320-wide tiles against tile_cfg 28
@pytest.mark.parametrize("cfg", [34, 35])
@pytest.mark.parametrize("K", [64, 160])
def test_320_wide_geglu_tiles_are_bitwise_tile_28(ops, cfg, K):
    """GEGLU + folded LayerNorm + out_ps at M = 288, N = 704: one full and one partial row tile (two full and one partial at
    128 rows), two full column tiles and a 64-wide edge, a ring longer (K = 64: 4 stages) and shorter (K = 160) than K."""
    p = geglu_problem(ops, 288, 704, K, 900 + K)
    full = None
    for with_fp32 in (True, False):
        ref = run3(lambda: launch_geglu(ops, p, 28, with_fp32))
        got = run3(lambda: launch_geglu(ops, p, cfg, with_fp32))
        same(got, ref, f"tile {cfg} K={K} fp32 output {with_fp32}")
        full = full or got
        assert torch.equal(got["out_ps"], ops.pack_ps(full["out"].contiguous(), h2_flag=p["flag"]).view(-1))


@pytest.mark.parametrize("cfg", [34, 35])
def test_320_wide_tiles_lane_column_form_is_bitwise_tile_28(ops, cfg):
    """the lane = column epilogue (residual + per-sample vector + GroupNorm records) at M = 160, N = 320, K = 96"""
    p = rows_problem(ops, 160, 320, 96, True, 920)
    ref = run3(lambda: launch_rows(ops, p, 28, 1, "col"))
    got = run3(lambda: launch_rows(ops, p, cfg, 1, "col"))
    same(got, ref, f"tile {cfg}")


# ------------------------------------------------------------------------------------------ 2. K groups against splitk = 2
@pytest.mark.parametrize("h2", [True, False], ids=["f16x2", "bf16x3"])
@pytest.mark.parametrize("form", ["tr", "col"])
@pytest.mark.parametrize("K,k0", [(96, 0), (32, 0), (96, 32)])
def test_k_groups_are_bitwise_split_k_2_rows(ops, K, k0, form, h2):
    """M = 160, N = 160: K = 96 gives slices of 2 and 1 chunks, K = 32 an empty second slice (reference: see the module text); k0 = 32: two A sources whose seam lies inside the first slice."""
    p = rows_problem(ops, 160, 160, K, h2, 940 + K + k0)
    pref = p
    if K == 32:      # the same product as slice 0 of a K = 64 problem whose second slice sums zeros
        pref = dict(p, K=64, wp=torch.cat([p["wp"], torch.zeros_like(p["wp"])]).contiguous())
        pref["wps"] = ops.pack_wps(pref["wp"], h2=h2)
        if h2:       # (one scale for the weight, zeros or not)
            assert ops.h2_scale_exp(pref["wp"]) == ops.h2_scale_exp(p["wp"])
        pref["a_ps"] = ops.pack_ps(torch.cat([p["x"], torch.zeros_like(p["x"])], 1).contiguous(), h2_flag=p["flag"] if h2 else None)
    ref = run3(lambda: launch_rows(ops, pref, 27, 2, form))
    got = run3(lambda: launch_rows(ops, p, 40, 1, form))
    same(got, ref, f"tile 40 K={K} k0={k0} {form}")


@pytest.mark.parametrize("stride,records", [(1, False), (1, True), (2, False)])
def test_k_groups_are_bitwise_split_k_2_conv(ops, stride, records):
    """conv mode: n = 2, 8x8, 64 -> 160 channels (one 32-channel chunk per group), bias + per-sample vector + residual"""
    n, h, w, cin, cout = 2, 8, 8, 64, 160
    oh = (h + 2 - 3) // stride + 1
    x = rnd(960, n * h * w, cin).cuda()
    wt = (rnd(961, cout, cin, 3, 3) / np.sqrt(9 * cin)).cuda()
    wp = ops.pack_conv3x3(wt)
    flag = flag_()
    wps, y_ps = ops.pack_wps(wp, h2=True), ops.pack_ps(x, h2_flag=flag)
    bias, vec, res = (0.1 * rnd(962, cout)).cuda(), rnd(963, n, cout).cuda(), rnd(964, n, oh, oh, cout).cuda()
    assert not records or (oh * oh) % 32 == 0        # (records need whole 32-row tiles inside a sample: stride 1 here)

    def launch(cfg, sk):
        checks = []
        out, c = padded((n, oh, oh, cout))
        checks.append(c)
        ws = rec = None
        if sk > 1:
            ws, c = padded((sk * n * oh * oh * cout,))
            checks.append(c)
        if records:
            rec, c = padded((n * oh * oh // 32, cout, 3))
            checks.append(c)
        ops.conv3x3_ps(y_ps, n, h, w, cin, wp, wps, flag, bias=bias, stride=stride, batch_vec=vec, residual=res, out=out, tile_cfg=cfg,
                       splitk=sk, splitk_ws=ws, stats_out=rec)
        torch.cuda.synchronize()
        for c in checks:
            c()
        return dict(out=out, records=rec) if records else dict(out=out)

    ref = run3(lambda: launch(27, 2))
    got = run3(lambda: launch(40, 1))
    assert int(flag.item()) == 0
    same(got, ref, f"conv stride {stride} records {records}")


# ------------------------------------------------------------------------------------------ 3. the epilogues split-K cannot run
def test_k_groups_geglu_and_out_ps_against_float64(ops):
    """tile_cfg 48 (128x320 with two K groups, the hand-over in two passes): GEGLU + folded LayerNorm, fp32 output and out_ps, at
    M = 160, N = 704, K = 96 against float64 under the GEGLU bound of tests/test_f16x2_gpu.py (class of the fp32 form, floor 3e-6);
    out_ps is exactly the split of the fp32 output."""
    p = geglu_problem(ops, 160, 704, 96, 980)
    inner = p["N"] // 2
    xn = F.layer_norm(p["x"].double(), (p["K"],), p["g"].double(), p["be"].double(), 1e-5)
    hcat = xn @ p["w"].double().t() + p["b"].double()
    ref = hcat[:, :inner] * F.gelu(hcat[:, inner:])
    y32 = ops.linear(p["x"].cuda(), p["w2"], p["b2"], row_stats=p["st"], ln_colsum=p["cs"], geglu=True)
    got = run3(lambda: launch_geglu(ops, p, 48))
    f16x2_class(err(y32, ref), err(got["out"], ref), 3e-6, "GEGLU on tile 48")
    assert torch.equal(got["out_ps"], ops.pack_ps(got["out"].contiguous(), h2_flag=p["flag"]).view(-1))
    only_ps = run3(lambda: launch_geglu(ops, p, 48, with_fp32=False))
    assert torch.equal(only_ps["out_ps"], got["out_ps"])
    # the same sum as the 128x320 tile without groups, up to the order of the two slices: the same error class
    f16x2_class(err(y32, ref), err(launch_geglu(ops, p, 35)["out"], ref), 3e-6, "GEGLU on tile 35")


def test_k_groups_out_ps_on_the_128x160_tile_against_float64(ops):
    """tile_cfg 40 with residual and out_ps (M = 160, N = 160, K = 96; the linear bound of tests/test_f16x2_gpu.py: floor 2e-6)"""
    p = rows_problem(ops, 160, 160, 96, True, 990)
    M, N, K = p["M"], p["N"], p["K"]
    ref = p["x"].double().cpu() @ p["w"].double().cpu().t() + p["bias"].double().cpu() + p["res"].double().cpu()
    y32 = ops.linear(p["x"], p["wp"], p["bias"], residual=p["res"])

    def launch():
        out, c0 = padded((M, N))
        o_ps, c1 = padded_ps(ops, M, N, True)
        ops.igemm(ops.make_igemm_args(M, N, K, None, K, p["wp"], out, N, M, tile_cfg=40, splitk=1, a_ps=p["a_ps"], w_ps=p["wps"], out_ps=o_ps,
                                      range_flag=p["flag"], bias=p["bias"], residual=p["res"]))
        torch.cuda.synchronize()
        c0()
        c1()
        return dict(out=out, out_ps=o_ps)
    got = run3(launch)
    assert int(p["flag"].item()) == 0
    f16x2_class(err(y32, ref), err(got["out"], ref), 2e-6, "residual + out_ps on tile 40")
    assert torch.equal(got["out_ps"], ops.pack_ps(got["out"].contiguous(), h2_flag=p["flag"]).view(-1))


def test_k_groups_qkv_projection_writes_the_attention_kv_tiles(ops):
    """tile_cfg 40 with attn_kv_out: 2 samples of 64 tokens, 5 heads (M = 128, N = 480, K = 160).  q third: fp32, against float64
    in the class of the fp32 form; the K / V tiles: bit for bit what the attention's own pre-pass makes of this tile's fp32 K / V
    (the statement of tests/test_f16x2_gpu.py for tile_cfg 23 / 27)."""
    from dsml_thesis_amd import lib as L
    n, tokens, heads = 2, 64, 5
    C_ = heads * 32
    M, K, N = n * tokens, C_, 3 * C_
    x = rnd(1000, M, K) + 0.3 * rnd(1001, M, 1)
    w, b = rnd(1002, N, K) / np.sqrt(K), 0.1 * rnd(1003, N)
    g, be = 1 + 0.2 * rnd(1004, K), 0.2 * rnd(1005, K)
    wp = ops.pack_linear(w.cuda())
    w2, cs, b2 = ops.fold_layernorm(wp, g.cuda(), be.cuda(), b.cuda())
    flag = flag_()
    st, xps = ops.ln_stats_ps(x.cuda(), h2_flag=flag)
    wps = ops.pack_wps(w2, h2=True)
    kw = dict(tf=L.TF_LAYERNORM_FOLDED, row_stats=st, ln_colsum=cs, bias=b2, tile_cfg=40, splitk=1, a_ps=xps, w_ps=wps, range_flag=flag)
    nkv = L.load().ldmk_attn_kv_split_h2_bytes(n, tokens, heads)

    def launch(with_kv):
        out, c0 = padded((M, N), fill=7.0)
        kv, c1 = padded((nkv,), torch.uint8, fill=0)
        ops.igemm(ops.make_igemm_args(M, N, K, None, K, w2, out, N, tokens, attn_kv=(kv, tokens, heads) if with_kv else None, **kw))
        torch.cuda.synchronize()
        c0()
        c1()
        return dict(out=out, kv=kv)
    plain = run3(lambda: launch(False))
    got = run3(lambda: launch(True))
    assert torch.equal(got["out"][:, :C_], plain["out"][:, :C_]) and bool((got["out"][:, C_:] == 7.0).all())      # K / V are not stored as fp32
    kv_ref, att = torch.zeros(nkv, device="cuda", dtype=torch.uint8), torch.empty(M, C_, device="cuda")
    L.call("ldmk_attn_self_h2", plain["out"].data_ptr(), kv_ref.data_ptr(), att.data_ptr(), flag.data_ptr(), n, tokens, heads, 32 ** -0.5, ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(got["kv"], kv_ref) and int(flag.item()) == 0
    xn = F.layer_norm(x.double(), (K,), g.double(), be.double(), 1e-5)
    ref = xn @ w.double().t() + b.double()
    y32 = ops.linear(x.cuda(), w2, b2, row_stats=st, ln_colsum=cs)
    f16x2_class(err(y32, ref), err(plain["out"], ref), 2e-6, "QKV projection on tile 40")


# ------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_name_their_reason(ops):
    from dsml_thesis_amd import lib as L
    M, K, N = 64, 64, 64
    x, w = rnd(1020, M, K).cuda(), rnd(1021, K, N).cuda().contiguous()
    flag = flag_()
    out = torch.empty(M, N, device="cuda")
    ws = torch.empty(2 * M * N, device="cuda")
    xh, wh = ops.pack_ps(x, h2_flag=flag), ops.pack_wps(w, h2=True)
    with pytest.raises(L.LdmkError, match="take the place of split-K"):            # K groups and split-K over workgroups
        ops.igemm(ops.make_igemm_args(M, N, K, None, K, w, out, N, M, tile_cfg=40, splitk=2, splitk_ws=ws, a_ps=xh, w_ps=wh, range_flag=flag))
    for cfg in (36, 37, 38, 39, 41, 47):                                            # K groups on the eight-wave tiles
        with pytest.raises(L.LdmkError, match="eight-wave"):
            ops.igemm(ops.make_igemm_args(M, N, K, None, K, w, out, N, M, tile_cfg=cfg, splitk=1, a_ps=xh, w_ps=wh, range_flag=flag))
    x3, w3 = ops.pack_ps(x), ops.pack_wps(w)
    for cfg in (34, 35, 48):                                                        # the 320-wide tiles in bf16x3
        with pytest.raises(L.LdmkError, match="f16x2 arithmetic only"):
            ops.igemm(ops.make_igemm_args(M, N, K, None, K, w, out, N, M, tile_cfg=cfg, splitk=1, a_ps=x3, w_ps=w3))
    wo = rnd(1022, K, 96).cuda().contiguous()                                      # GEGLU on three 32-column tiles
    who = ops.pack_wps(wo, h2=True)
    for cfg in (34, 35, 48):
        with pytest.raises(L.LdmkError, match="N%64==0"):
            ops.igemm(ops.make_igemm_args(M, 96, K, None, K, wo, torch.empty(M, 48, device="cuda"), 48, M, epi=L.EPI_GEGLU, tile_cfg=cfg, splitk=1,
                                          a_ps=xh, w_ps=who, range_flag=flag))
    torch.cuda.synchronize()
    ops.igemm(ops.make_igemm_args(M, N, K, None, K, w, out, N, M, tile_cfg=40, splitk=1, a_ps=xh, w_ps=wh, range_flag=flag))      # and what runs, runs
    torch.cuda.synchronize()
