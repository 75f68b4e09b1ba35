"""GPU: the other arm of every A/B switch the LIBRARY reads (dsml_thesis_amd/switches.py, scope "library"), at op level, held to
the contract its table line states.  The library latches its switches from the environment once per process; the tests reach
the other arm in this process through ldmk_switch_override (include/ldmk.h), always taken back in a `finally`, and first ask
ldmk_switch_value which arm they are running.  Both arms must meet the float64 bound the existing test of that kernel uses
(quoted where it is applied); where the table says "same bits" they must also be torch.equal, GroupNorm records and PS-layout
results included.  Shapes are the smallest at which the arm can differ: the launchers' own predicates are recomputed from the
tile sizes and asserted, so that a change of a predicate cannot make a test vacuous.  tests/test_switch_arms_cpu.py keeps ARMS
complete."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rnd
from test_f16x2_gpu import _attention_ref, _f16x2_class, lazy_maximum_scores
from test_ops_gpu import WINOGRAD_CASES, close, nchw, nhwc, ops, winograd_case  # noqa: F401  (the `ops` fixture)
from test_split_gpu import _err, _same_class

pytestmark = pytest.mark.gpu

# switch -> the tests that run its other arm
ARMS = {
    "LDMK_IG_NFAST": ["test_switch_arms_gpu::test_lds_tiled_igemm_arms_rows", "test_switch_arms_gpu::test_lds_tiled_igemm_arms_conv",
                      "test_switch_arms_gpu::test_lds_tiled_igemm_arms_b_trans_and_general_only_forms"],
    "LDMK_IG_LEAN": ["test_switch_arms_gpu::test_lds_tiled_igemm_arms_rows", "test_switch_arms_gpu::test_lds_tiled_igemm_arms_conv",
                     "test_switch_arms_gpu::test_lds_tiled_igemm_arms_b_trans_and_general_only_forms"],
    "LDMK_PS_NFAST": ["test_switch_arms_gpu::test_pre_split_tile_arms_rows", "test_switch_arms_gpu::test_pre_split_tile_arms_geglu",
                      "test_switch_arms_gpu::test_pre_split_tile_arms_conv"],
    "LDMK_PS_LEAN": ["test_switch_arms_gpu::test_pre_split_tile_arms_rows", "test_switch_arms_gpu::test_pre_split_tile_arms_geglu",
                     "test_switch_arms_gpu::test_pre_split_tile_arms_conv"],
    "LDMK_ATTN_QB": ["test_switch_arms_gpu::test_attention_query_blocks_per_wave"],
    "LDMK_ATTN_PIPE": ["test_switch_arms_gpu::test_attention_key_loop_forms", "test_switch_arms_gpu::test_attention_key_loop_forms_on_ordered_scores"],
    "LDMK_ATTN_XCD": ["test_switch_arms_gpu::test_attention_workgroup_order"],
    "LDMK_WGRAD_TR": ["test_switch_arms_gpu::test_bf16_weight_gradient_with_the_strided_gather"],
    "LDMK_WINO_STAGED": ["test_switch_arms_gpu::test_winograd_first_transforms"],
}


@pytest.fixture
def arm():
    """arm(name, value): a context in which the library switch `name` has `value` (None: whatever the environment / default gives);
    asserts that the library reports that value, and takes the override back on the way out."""
    from dsml_thesis_amd import lib, switches
    so = lib.load()
    touched = set()

    @contextlib.contextmanager
    def _arm(name, value):
        assert switches.SWITCHES[name][1] == "library"
        key = name.encode()
        touched.add(key)
        assert so.ldmk_switch_override(key, -1 if value is None else value) >= 0
        try:
            want = int(switches.get(name, switches.SWITCHES[name][0]) or 0) if value is None else value
            assert so.ldmk_switch_value(key) == want, (name, value, so.ldmk_switch_value(key))
            yield
        finally:
            so.ldmk_switch_override(key, -1)
    yield _arm
    for key in touched:
        so.ldmk_switch_override(key, -1)


def _flag():
    return torch.zeros(1, device="cuda", dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# LDMK_IG_NFAST / LDMK_IG_LEAN: the LDS-tiled implicit GEMM (csrc/igemm.hip)
IG_TILE = {1: (128, 128), 2: (64, 128), 3: (64, 64), 4: (64, 64), 5: (128, 160), 6: (64, 160)}       # tile_cfg -> BM, BN (dispatch())
IG_WAVE = {1: (64, 64), 2: (32, 64), 3: (64, 64), 4: (32, 32), 5: (32, 160), 6: (32, 160)}            # rows x columns of one wave tile
IG_FORMS = [("f32", c) for c in (1, 2, 3, 4, 5, 6)] + [(f, c) for f in ("bf16", "bf16x3", "f16x2") for c in (1, 2, 4, 5)]
OPERANDS = ["none", "vec", "res", "both"]           # the four operand sets of ig_lean_epilogue / col_lean


def _nfast_taken(M, N, BM, BN, b_trans=False):
    """the launchers' predicate (launch_cfg_g; ps_launch and psc_launch without the b_trans term)"""
    return (not b_trans) and -(-N // BN) > 1 and -(-M // BM) >= 8


def _interior_and_ragged(M, N, BM, BN, WM, WN):
    """at least one wave tile wholly inside M x N (the lean forms' domain) and a ragged last tile in both directions"""
    return M >= WM and N >= WN and M % BM != 0 and N % BN != 0


def _ig_compute(ops, form, wp):
    """compute code, the extra make_igemm_args of the form, and its (rtol, atol) against float64 -- of the existing tests:
    test_ops_gpu.test_conv3x3 (f32: 1e-4), test_split_gpu.test_split_linear_matches_float64_like_the_fp32_form (bf16x3: 3e-6; 6e-6
    with a per-sample vector as a fourth fp32 term: test_warp_specialised_tiles_..., applied by the caller), test_f16x2_gpu.test_f16x2_linear_... (6e-6),
    test_bf16_gpu.test_bf16_linear_forward_and_dgrad_form (bf16: 2e-5 against the product of the bf16-rounded operands)."""
    from dsml_thesis_amd import lib as L
    if form == "f32":
        return dict(compute=L.COMPUTE_F32), (1e-4, 1e-4)
    if form == "bf16":
        return dict(compute=L.COMPUTE_BF16), (2e-5, 2e-5)
    if form == "bf16x3":
        ops.pack_wsplit(wp)
        return dict(compute=L.COMPUTE_BF16X3), (3e-6, 3e-6)
    ops.pack_wsplit_h2(wp)
    return dict(compute=L.COMPUTE_F16X2, range_flag=_flag()), (6e-6, 6e-6)


def _bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _run_both(arm, name, other, launch):
    """launch() under the default arm and under `name` = other; the two results (tuples of tensors or None) must be bit-equal"""
    with arm(name, None):
        base = launch()
    with arm(name, other):
        got = launch()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(base, got)):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b), f"{name}={other}: result {i} differs from the default arm in {int((a != b).sum())} of {a.numel()} elements"
    return base


def _operand_kw(opnd, M, N, rps, seed):
    """(make_igemm_args operands, float64 sum of what the epilogue adds)"""
    kw, add = {}, torch.zeros(M, N, dtype=torch.float64)
    if opnd in ("vec", "both"):
        vec = rnd(seed, -(-M // rps), N)
        kw.update(batch_vec=vec.cuda(), batch_vec_ld=N)
        add = add + vec.double().repeat_interleave(rps, 0)[:M]
    if opnd in ("res", "both"):
        res = rnd(seed + 1, M, N)
        kw.update(residual=res.cuda())
        add = add + res.double()
    return kw, add


@pytest.mark.parametrize("form,cfg", IG_FORMS)
def test_lds_tiled_igemm_arms_rows(ops, arm, form, cfg):
    """Rows mode, M = 8 BM + 40 (nine row tiles, the last ragged) and 8 BM + 96 (a multiple of 32: GroupNorm records), N = BN + 32
    (two column tiles, the last partial), K = 96, split-K 1 and 2, the four operand sets with and without records: LDMK_IG_NFAST=0
    (row-major tile order) and LDMK_IG_LEAN=0 (the general epilogue on interior wave tiles) give the default arm's bits."""
    BM, BN = IG_TILE[cfg]
    K, N = 96, BN + 32
    w, b = rnd(901, N, K) / np.sqrt(K), 0.1 * rnd(902, N)
    wp, bc = ops.pack_linear(w.cuda()), b.cuda()
    ckw, tol = _ig_compute(ops, form, wp)
    if form == "bf16":
        ckw["w_bf16t"] = ops.pack_wbf16t(wp)             # (the training step's form: the pre-packed bf16 image)
    for M in (8 * BM + 40, 8 * BM + 96):
        assert _nfast_taken(M, N, BM, BN) and _interior_and_ragged(M, N, BM, BN, *IG_WAVE[cfg])
        x = rnd(900, M, K)
        xc = x.cuda()
        prod = (_bf16r(x).double() @ _bf16r(w).double().t()) if form == "bf16" else x.double() @ w.double().t()
        for opnd in OPERANDS:
            okw, add = _operand_kw(opnd, M, N, 64, 903)
            ref = (prod + b.double() + add).float()
            for sk in (1, 2):
                for stats in ((False, True) if M % 32 == 0 else (False,)):
                    ws = torch.empty(sk * M * N, device="cuda") if sk > 1 else None

                    def launch():
                        out = torch.full((M, N), float("nan"), device="cuda")
                        rec = torch.zeros(M // 32, N, 3, device="cuda") if stats else None
                        a = ops.make_igemm_args(M, N, K, xc, K, wp, out, N, 64, bias=bc, tile_cfg=cfg, splitk=sk, splitk_ws=ws, **okw, **ckw)
                        if stats:
                            a.stats_out = rec.data_ptr()
                        ops.igemm(a)
                        return out, rec
                    for name in ("LDMK_IG_NFAST", "LDMK_IG_LEAN"):
                        out, _ = _run_both(arm, name, 0, launch)
                    close(out, ref, *((6e-6, 6e-6) if form == "bf16x3" and "batch_vec" in okw else tol))
    if "range_flag" in ckw:
        assert int(ckw["range_flag"].item()) == 0


@pytest.mark.parametrize("form,cfg", IG_FORMS)
def test_lds_tiled_igemm_arms_conv(ops, arm, form, cfg):
    """Conv mode: a 3x3 convolution of 32 channels on a 33 x 32 image (1056 output rows >= 8 BM + 1: nine row tiles for the 128-row
    tiles, seventeen for the 64-row ones, the last ragged), BN + 32 output channels, K = 288, split-K 1 and 2."""
    BM, BN = IG_TILE[cfg]
    n, cin, h, w_ = 1, 32, 33, 32
    cout, M, K = BN + 32, n * h * w_, 9 * cin
    assert M >= 8 * BM + 1 and _nfast_taken(M, cout, BM, BN) and _interior_and_ragged(M, cout, BM, BN, *IG_WAVE[cfg])
    x, wt, b = rnd(910, n, cin, h, w_), rnd(911, cout, cin, 3, 3) / np.sqrt(K), 0.1 * rnd(912, cout)
    wp, bc, xc = ops.pack_conv3x3(wt.cuda()), b.cuda(), nhwc(x)
    ckw, tol = _ig_compute(ops, form, wp)
    okw, add = _operand_kw("both", M, cout, h * w_, 913)
    xr, wr = (_bf16r(x), _bf16r(wt)) if form == "bf16" else (x, wt)
    ref = nhwc(F.conv2d(xr.double(), wr.double(), b.double(), padding=1).cpu()).cpu().reshape(M, cout) + add
    y32 = torch.empty(M, cout, device="cuda")
    ops.igemm(ops.make_igemm_args(M, cout, K, xc, cin, wp, y32, cout, h * w_, conv=(h, w_, h, w_, 1, 1, 0), bias=bc, tile_cfg=cfg, splitk=1, **okw))
    e32 = _err(y32, ref)
    for sk in (1, 2):
        for stats in (False, True):
            ws = torch.empty(sk * M * cout, device="cuda") if sk > 1 else None

            def launch():
                out = torch.full((M, cout), float("nan"), device="cuda")
                rec = torch.zeros(M // 32, cout, 3, device="cuda") if stats else None
                a = ops.make_igemm_args(M, cout, K, xc, cin, wp, out, cout, h * w_, conv=(h, w_, h, w_, 1, 1, 0), bias=bc, tile_cfg=cfg,
                                        splitk=sk, splitk_ws=ws, **okw, **ckw)
                if stats:
                    a.stats_out = rec.data_ptr()
                ops.igemm(a)
                return out, rec
            for name in ("LDMK_IG_NFAST", "LDMK_IG_LEAN"):
                out, _ = _run_both(arm, name, 0, launch)
            if form in ("f32", "bf16"):
                close(out, ref.float(), *tol)
            else:       # test_split_gpu.test_split_conv3x3_... / test_f16x2_gpu.test_f16x2_conv3x3_...: the class of the fp32 form, floor 3e-6
                (_same_class if form == "bf16x3" else _f16x2_class)(e32, _err(out, ref), 3e-6)


def test_lds_tiled_igemm_arms_b_trans_and_general_only_forms(ops, arm):
    """(a) b_trans (the weight as [N][K]): the tile-order predicate is false whatever the shape, so LDMK_IG_NFAST cannot matter;
    (b) folded LayerNorm, (c) GEGLU: the general epilogue in both arms of LDMK_IG_LEAN (split-K: the rows-mode test).  All equal."""
    from dsml_thesis_amd import lib as L
    BM, BN = IG_TILE[1]
    M, N, K = 8 * BM + 40, BN + 32, 96
    x, w, b = rnd(920, M, K) + 0.3, rnd(921, N, K) / np.sqrt(K), 0.1 * rnd(922, N)
    xc, wc, bc = x.cuda(), w.cuda().contiguous(), b.cuda()
    assert not _nfast_taken(M, N, BM, BN, b_trans=True) and _nfast_taken(M, N, BM, BN)

    def bt():
        out = torch.empty(M, N, device="cuda")
        ops.igemm(ops.make_igemm_args(M, N, K, xc, K, wc, out, N, M, b_trans=True, bias=bc, tile_cfg=1, splitk=1))
        return (out,)
    for name in ("LDMK_IG_NFAST", "LDMK_IG_LEAN"):
        out, = _run_both(arm, name, 0, bt)
    close(out, (x.double() @ w.double().t() + b.double()).float(), 1e-4, 1e-4)
    g, be = 1 + 0.2 * rnd(923, K), 0.2 * rnd(924, K)
    st = ops.ln_stats(xc)
    xn = F.layer_norm(x.double(), (K,), g.double(), be.double(), 1e-5)
    w2, cs, b2 = ops.fold_layernorm(ops.pack_linear(wc), g.cuda(), be.cuda(), bc)

    def lnf():
        out = torch.empty(M, N, device="cuda")
        ops.igemm(ops.make_igemm_args(M, N, K, xc, K, w2, out, N, M, tf=L.TF_LAYERNORM_FOLDED, row_stats=st, ln_colsum=cs, bias=b2, tile_cfg=1,
                                      splitk=1))
        return (out,)
    for name in ("LDMK_IG_NFAST", "LDMK_IG_LEAN"):
        out, = _run_both(arm, name, 0, lnf)
    close(out, (xn @ w.double().t() + b.double()).float(), 1e-4, 1e-4)
    Ng = 2 * N                                          # (value, gate) column pairs: 320 packed columns, three 128-wide tiles
    wg, bg = rnd(925, Ng, K) / np.sqrt(K), 0.1 * rnd(926, Ng)
    wpg, bpg = ops.pack_geglu(wg.cuda(), bg.cuda())
    w3, cs3, b3 = ops.fold_layernorm(wpg, g.cuda(), be.cuda(), bpg)

    def geglu():
        out = torch.empty(M, Ng // 2, device="cuda")
        ops.igemm(ops.make_igemm_args(M, Ng, K, xc, K, w3, out, Ng // 2, M, tf=L.TF_LAYERNORM_FOLDED, row_stats=st, ln_colsum=cs3, bias=b3,
                                      epi=L.EPI_GEGLU, tile_cfg=1, splitk=1))
        return (out,)
    for name in ("LDMK_IG_NFAST", "LDMK_IG_LEAN"):
        out, = _run_both(arm, name, 0, geglu)
    y = xn @ wg.double().t() + bg.double()
    close(out, (y[:, :Ng // 2] * F.gelu(y[:, Ng // 2:])).float(), 1e-4, 1e-4)


# ---------------------------------------------------------------------------------------------------------------------------------
# LDMK_PS_NFAST / LDMK_PS_LEAN: the pre-split tiles (csrc/igemm_ps.hip), both launchers (ps_launch, psc_launch)
PS_TILE = {23: (256, 160), 24: (256, 320), 25: (256, 256), 26: (128, 320), 27: (128, 160), 28: (128, 256), 29: (256, 160), 30: (256, 128),
           31: (256, 160), 32: (256, 128), 33: (128, 256)}                                          # kPsCfg
PS_WARP_SPECIALISED = (29, 30)       # pw_launch consults neither switch: the arms are one launch (asserted equal like the others)


def _ps_pack(ops, x, wp, h2, flag):
    if h2:
        return ops.pack_ps(x, h2_flag=flag), ops.pack_wps(wp, h2=True)
    return ops.pack_ps(x), ops.pack_wps(wp)


def _ps_forms(cfgs):
    """(tile_cfg, F16X2?) pairs: the warp-specialised tiles exist in the bf16x3 arithmetic only (igemm_ps_unsupported)"""
    return [pytest.param(c, h2, id=f"{c}-{'f16x2' if h2 else 'bf16x3'}") for c in cfgs for h2 in (False, True) if not (h2 and c in PS_WARP_SPECIALISED)]


@pytest.mark.parametrize("cfg,h2", _ps_forms([23, 24, 26, 27, 29, 31]))
def test_pre_split_tile_arms_rows(ops, arm, cfg, h2):
    """Rows mode, M = 8 BM + 40 / 8 BM + 96, N = BN + 32, K = 96, split-K 1 and 2.  Operand sets of ps_epilogue: the transposed form
    (no records) has lean copies for residual, neither, residual + vector and folded LayerNorm without residual; a vector alone takes
    the general form in both arms; with GroupNorm records (lane = column form, col_lean) the four sets of the LDS-tiled kernel.
    Bounds: test_ps_gpu.test_ps_gemm_is_bitwise_the_lds_tiled_bf16x3_gemm (5e-6), test_f16x2_gpu.test_f16x2_linear_... (6e-6);
    folded LayerNorm: test_ps_gpu.test_ps_gemm_geglu_with_folded_layernorm_and_split_output (2e-5)."""
    from dsml_thesis_amd import lib as L
    BM, BN = PS_TILE[cfg]
    K, N = 96, BN + 32
    w, b = rnd(931, N, K) / np.sqrt(K), 0.1 * rnd(932, N)
    wp, bc = ops.pack_linear(w.cuda()), b.cuda()
    flag = _flag()
    tol = (6e-6, 6e-6) if h2 else (5e-6, 5e-6)
    g, be = 1 + 0.2 * rnd(935, K), 0.2 * rnd(936, K)
    w2, cs, b2 = ops.fold_layernorm(wp, g.cuda(), be.cuda(), bc)
    for M in (8 * BM + 40, 8 * BM + 96):
        assert _nfast_taken(M, N, BM, BN) and _interior_and_ragged(M, N, BM, BN, 32, 32)
        x = rnd(930, M, K) + 0.3 * rnd(937, M, 1)
        xps, wps = _ps_pack(ops, x.cuda(), wp, h2, flag)
        prod = x.double() @ w.double().t() + b.double()
        for opnd in OPERANDS + ["lnf"]:
            if opnd == "lnf":
                st, xuse = ops.ln_stats_ps(x.cuda(), h2_flag=flag) if h2 else ops.ln_stats_ps(x.cuda())
                okw = dict(tf=L.TF_LAYERNORM_FOLDED, row_stats=st, ln_colsum=cs, bias=b2, w_ps=ops.pack_wps(w2, h2=h2))
                wuse = w2
                ref = (F.layer_norm(x.double(), (K,), g.double(), be.double(), 1e-5) @ w.double().t() + b.double()).float()
            else:
                okw, add = _operand_kw(opnd, M, N, 64, 933)
                okw.update(bias=bc, w_ps=wps)
                wuse, xuse = wp, xps
                ref = (prod + add).float()
            for sk in (1, 2):
                for stats in ((False, True) if (M % 32 == 0 and opnd != "lnf") else (False,)):
                    ws = torch.empty(sk * M * N, device="cuda") if sk > 1 else None

                    def launch():
                        out = torch.full((M, N), float("nan"), device="cuda")
                        rec = torch.zeros(M // 32, N, 3, device="cuda") if stats else None
                        a = ops.make_igemm_args(M, N, K, None, K, wuse, out, N, 64, tile_cfg=cfg, splitk=sk, splitk_ws=ws, a_ps=xuse, range_flag=flag,
                                                **okw)
                        assert a.compute == (L.COMPUTE_F16X2 if h2 else L.COMPUTE_BF16X3)
                        if stats:
                            a.stats_out = rec.data_ptr()
                        ops.igemm(a)
                        return out, rec
                    for name in ("LDMK_PS_NFAST", "LDMK_PS_LEAN"):
                        out, _ = _run_both(arm, name, 0, launch)
                    close(out, ref, *((2e-5, 2e-5) if opnd == "lnf" else tol))
    assert int(flag.item()) == 0


@pytest.mark.parametrize("cfg,h2", _ps_forms([25, 28, 30, 32, 33]))
def test_pre_split_tile_arms_geglu(ops, arm, cfg, h2):
    """The GEGLU projection with folded LayerNorm (lean copy 1 of the transposed epilogue), fp32 and PS-layout results: both
    switches, bit for bit; float64 bound of test_ps_gpu.test_ps_gemm_geglu_with_folded_layernorm_and_split_output (2e-5)."""
    from dsml_thesis_amd import lib as L
    BM, BN = PS_TILE[cfg]
    M, K, N = 8 * BM + 96, 96, BN + 64                    # (packed (value, gate) pairs: N / 2 result columns; out_ps: whole row blocks)
    assert _nfast_taken(M, N, BM, BN) and _interior_and_ragged(M, N, BM, BN, 32, 64)
    x = rnd(940, M, K) + 0.5 * rnd(941, M, 1)
    w, b = rnd(942, N, K) / np.sqrt(K), 0.1 * rnd(943, N)
    g, be = 1 + 0.2 * rnd(944, K), 0.2 * rnd(945, K)
    wp, bp = ops.pack_geglu(w.cuda(), b.cuda())
    w2, cs, b2 = ops.fold_layernorm(wp, g.cuda(), be.cuda(), bp)
    flag = _flag()
    st, xps = ops.ln_stats_ps(x.cuda(), h2_flag=flag) if h2 else ops.ln_stats_ps(x.cuda())
    wps = ops.pack_wps(w2, h2=h2)

    def launch():
        out = torch.full((M, N // 2), float("nan"), device="cuda")
        out_ps = ops.ps_empty(M, N // 2, h2=h2)
        a = ops.make_igemm_args(M, N, K, None, K, w2, out, N // 2, M, tf=L.TF_LAYERNORM_FOLDED, row_stats=st, ln_colsum=cs, bias=b2,
                                epi=L.EPI_GEGLU, tile_cfg=cfg, splitk=1, a_ps=xps, w_ps=wps, out_ps=out_ps, range_flag=flag)
        ops.igemm(a)
        return out, out_ps
    for name in ("LDMK_PS_NFAST", "LDMK_PS_LEAN"):
        out, out_ps = _run_both(arm, name, 0, launch)
    assert torch.equal(out_ps, ops.pack_ps(out, h2_flag=flag) if h2 else ops.pack_ps(out))
    y = F.layer_norm(x.double(), (K,), g.double(), be.double(), 1e-5) @ w.double().t() + b.double()
    close(out, (y[:, :N // 2] * F.gelu(y[:, N // 2:])).float(), 2e-5, 2e-5)
    assert int(flag.item()) == 0


@pytest.mark.parametrize("cfg", [23, 24, 26, 27])
def test_pre_split_tile_arms_conv(ops, arm, cfg):
    """The conv-mode tile (psc_launch; F16X2 only): 32 channels on two 33 x 32 images (2112 output rows >= 8 BM + 1, ragged last
    row tile), BN + 32 output channels; the four operand sets, with and without GroupNorm records.  Float64 bound of
    test_ps_conv_gpu.test_conv_mode_ps_tile_is_bitwise_the_lds_tiled_f16x2_convolution (2e-5)."""
    BM, BN = PS_TILE[cfg]
    n, cin, h, w_ = 2, 32, 33, 32
    cout, M = BN + 32, n * h * w_
    assert M >= 8 * BM + 1 and M % 32 == 0 and (h * w_) % 32 == 0 and _nfast_taken(M, cout, BM, BN) and _interior_and_ragged(M, cout, BM, BN, 32, 32)
    x = nhwc(rnd(950, n, cin, h, w_)).contiguous()
    wt, b = rnd(951, cout, cin, 3, 3) / np.sqrt(9 * cin), 0.1 * rnd(952, cout)
    wp, bc = ops.pack_conv3x3(wt.cuda()), b.cuda()
    ops.pack_wsplit_h2(wp)
    wps, flag = ops.pack_wps(wp, h2=True), _flag()
    yps = ops.pack_ps(x.view(M, cin), h2_flag=flag)
    conv = nhwc(F.conv2d(nchw(x).double(), wt.double(), b.double(), padding=1)).cpu().reshape(M, cout)
    for opnd in OPERANDS:
        okw, add = _operand_kw(opnd, M, cout, h * w_, 953)
        for stats in (False, True):
            def launch():
                rec = torch.zeros(M // 32, cout, 3, device="cuda") if stats else None
                out = ops.conv3x3_ps(yps, n, h, w_, cin, wp, wps, flag, bias=bc, batch_vec=okw.get("batch_vec"), residual=okw.get("residual"),
                                     tile_cfg=cfg, stats_out=rec)
                return out.view(M, cout), rec
            for name in ("LDMK_PS_NFAST", "LDMK_PS_LEAN"):
                out, _ = _run_both(arm, name, 0, launch)
            close(out, (conv + add).float(), 2e-5, 2e-5)
    assert int(flag.item()) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# LDMK_ATTN_QB / LDMK_ATTN_PIPE / LDMK_ATTN_XCD: the pre-split attention kernels (csrc/attention_bf16.hip)
def _attn_all(ops, qkv, n, tokens, heads):
    """every entry point that reads LDMK_ATTN_QB on one input: name -> result (fp32 tensors and PS-layout bytes)"""
    from dsml_thesis_amd import lib as L
    so, C_, sc, st = L.load(), heads * 32, 32 ** -0.5, ops.stream()
    rows = n * tokens
    new = lambda: torch.full((rows, C_), float("nan"), device="cuda")
    kv3 = torch.empty(so.ldmk_attn_kv_split_bytes(n, tokens, heads), device="cuda", dtype=torch.uint8)
    kvh = torch.empty(so.ldmk_attn_kv_split_h2_bytes(n, tokens, heads), device="cuda", dtype=torch.uint8)
    flag = _flag()
    r = {"x3p": new(), "h2": new()}
    L.call("ldmk_attn_self_x3p", qkv.data_ptr(), kv3.data_ptr(), r["x3p"].data_ptr(), n, tokens, heads, sc, st)
    L.call("ldmk_attn_self_h2", qkv.data_ptr(), kvh.data_ptr(), r["h2"].data_ptr(), flag.data_ptr(), n, tokens, heads, sc, st)
    if tokens % 32 == 0:
        r.update({"x3p_ps": new(), "x3p_ps.ps": ops.ps_empty(rows, C_), "h2_ps": new(), "h2_ps.ps": ops.ps_empty(rows, C_, h2=True)})
        L.call("ldmk_attn_self_x3p_ps", qkv.data_ptr(), kv3.data_ptr(), r["x3p_ps"].data_ptr(), r["x3p_ps.ps"].data_ptr(), n, tokens, heads, sc, st)
        L.call("ldmk_attn_self_h2_ps", qkv.data_ptr(), kvh.data_ptr(), r["h2_ps"].data_ptr(), r["h2_ps.ps"].data_ptr(), flag.data_ptr(), n, tokens,
               heads, sc, st)
    if tokens % 64 == 0:      # (kvh: the tiles ldmk_attn_self_h2's pre-pass wrote -- what the fused QKV projection writes, test_f16x2_gpu)
        r.update({"h2_tiles": new(), "h2_tiles.ps": ops.ps_empty(rows, C_, h2=True)})
        L.call("ldmk_attn_self_h2_tiles", qkv.data_ptr(), kvh.data_ptr(), r["h2_tiles"].data_ptr(), r["h2_tiles.ps"].data_ptr(), flag.data_ptr(), n,
               tokens, heads, sc, st)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    return r


def _attn_bounds(r, ref, e32):
    """test_split_gpu.test_split_attention_matches_float64_like_the_fp32_kernel / test_f16x2_gpu.test_f16x2_attention_matches_float64_...:
    the class of the fp32 kernel against float64 (floor 2e-6) and 3e-6 element-wise"""
    for k, y in r.items():
        if k.endswith(".ps"):
            continue
        (_same_class if k.startswith("x3p") else _f16x2_class)(e32, _err(y, ref), 2e-6)
        close(y, ref.float(), 3e-6, 3e-6)


QB_CASES = [(n, t, h) for t in (64, 100, 130, 256, 257, 512) for n, h in ((3, 5), (1, 1))] + [(1, 2048, 1)]


@pytest.mark.parametrize("n,tokens,heads", QB_CASES)
def test_attention_query_blocks_per_wave(ops, arm, n, tokens, heads):
    """LDMK_ATTN_QB unset (one 32-query block per wave below 2048 tokens, two from there), 1 and 2 on ldmk_attn_self_x3p, _x3p_ps,
    _h2, _h2_ps and _h2_tiles: each within the float64 bounds of its kernel, and the same bits from all three -- with the one
    exception the table line states: two blocks per wave at a multiple of 256 tokens bring the F16X2 kernel's pipelined loop with
    them, whose lazy running maximum (LDMK_ATTN_PIPE=2, the default) is another arithmetic.  There the bits agree under
    LDMK_ATTN_PIPE=1 (the pipelined loop with the exact maximum), which is run for every case as well."""
    qkv = (1.5 * rnd(550, n * tokens, 3 * heads * 32)).cuda()
    ref = _attention_ref(qkv, n, tokens, heads)
    e32 = _err(ops.attn_self(qkv, n, tokens, heads), ref)
    res = {}
    for pipe in (None, 1):
        for qb in (None, 1, 2):
            with arm("LDMK_ATTN_PIPE", pipe), arm("LDMK_ATTN_QB", qb):
                res[pipe, qb] = _attn_all(ops, qkv, n, tokens, heads)
            _attn_bounds(res[pipe, qb], ref, e32)
        for qb in (1, 2):
            for k, want in res[pipe, None].items():
                if pipe is None and k.startswith("h2") and tokens % 256 == 0:
                    continue                                   # (the lazy maximum on one side only: held to the bounds above)
                assert torch.equal(res[pipe, qb][k], want), f"LDMK_ATTN_QB={qb} (LDMK_ATTN_PIPE={pipe}): {k} differs from the default"
        for k in ("x3p_ps", "h2_ps", "h2_tiles"):         # one kernel behind the plain and the PS entry points
            if k in res[pipe, None]:
                assert torch.equal(res[pipe, None][k], res[pipe, None][k.split("_")[0]])
    for k, want in res[None, None].items():               # LDMK_ATTN_PIPE=1 itself: the default's bits wherever the default does not pipeline
        if not (k.startswith("h2") and tokens % 256 == 0 and tokens >= 2048):
            assert torch.equal(res[1, None][k], want), k


def _h2_forms(ops, arm, qkv, n, tokens, heads):
    """ldmk_attn_self_h2_ps with two query blocks per wave under LDMK_ATTN_PIPE = 0, 1, 2: value -> (fp32 result, PS bytes)"""
    from dsml_thesis_amd import lib as L
    so = L.load()
    out = {}
    with arm("LDMK_ATTN_QB", 2):
        for pipe in (0, 1, 2):
            with arm("LDMK_ATTN_PIPE", pipe):
                y, ps, flag = torch.full((n * tokens, heads * 32), float("nan"), device="cuda"), ops.ps_empty(n * tokens, heads * 32, h2=True), _flag()
                kv = torch.empty(so.ldmk_attn_kv_split_h2_bytes(n, tokens, heads), device="cuda", dtype=torch.uint8)
                L.call("ldmk_attn_self_h2_ps", qkv.data_ptr(), kv.data_ptr(), y.data_ptr(), ps.data_ptr(), flag.data_ptr(), n, tokens, heads, 32 ** -0.5,
                       ops.stream())
                torch.cuda.synchronize()
                out[pipe] = (y, ps, int(flag.item()))
    return out


@pytest.mark.parametrize("tokens", [256, 512, 768, 320])
def test_attention_key_loop_forms(ops, arm, tokens):
    """LDMK_ATTN_PIPE with two query blocks per wave: at multiples of 256 tokens the pipelined key loop runs (2: lazy running
    maximum, 1: exact maximum) -- 1 gives the bits of the phase-separated loop (0), 2 stays in the F16X2 class against float64; at
    320 tokens no arm may pipeline and all three are one kernel."""
    n, heads = 2, 3
    qkv = (1.5 * rnd(550, n * tokens, 3 * heads * 32)).cuda()
    out = _h2_forms(ops, arm, qkv, n, tokens, heads)
    ref = _attention_ref(qkv, n, tokens, heads)
    e32 = _err(ops.attn_self(qkv, n, tokens, heads), ref)
    for pipe, (y, _, flagged) in out.items():
        assert flagged == 0
        _f16x2_class(e32, _err(y, ref), 2e-6)
        close(y, ref.float(), 3e-6, 3e-6)
    assert torch.equal(out[1][0], out[0][0]) and torch.equal(out[1][1], out[0][1]), "LDMK_ATTN_PIPE=1 promises the bits of LDMK_ATTN_PIPE=0"
    if tokens % 256:
        assert torch.equal(out[2][0], out[0][0]) and torch.equal(out[2][1], out[0][1])


def _largest_rise_over_the_row_maximum(qkv, n, tokens, heads):
    """float64: the most, in binary orders, by which a score of a 32-key block (from the second 64-key tile on, where the lazy loop
    starts) exceeds everything its row has seen before that block"""
    C_ = heads * 32
    q, k, _ = [t.reshape(n, tokens, heads, 32).permute(0, 2, 1, 3).double() for t in qkv.cpu().split(C_, dim=1)]
    s2 = q @ k.transpose(-1, -2) * (32 ** -0.5 * 1.4426950408889634)
    seen = torch.cummax(s2, dim=-1).values
    rise = max(float((s2[..., b:b + 32].max(-1).values - seen[..., b - 1]).max()) for b in range(64, tokens, 32))
    return rise


@pytest.mark.parametrize("order", ["rising", "steps", "peaked"])
def test_attention_key_loop_forms_on_ordered_scores(ops, arm, order):
    """The score orders of test_f16x2_attention_lazy_running_maximum at 512 tokens, two query blocks per wave: LDMK_ATTN_PIPE = 0 and
    1 (exact maximum) in the class of the fp32 kernel whatever the order, and the same bits; 2 (lazy maximum) in that class too --
    unless a block rises further above its row's maximum than the lazy loop's documented range (the fp32 exponential of the scaled
    probability, 2^(rise + 8) <= 2^100; the running maximum may lag the true one by the 7 orders between 2^8 and the 2^15 row-sum
    bound): then its range flag goes up and the result stays finite, as for an operand outside fp16's range.  At 512 tokens the
    one step of "steps" is such a rise (~50 binary orders for the average query, over 90 for some); at the 2048 tokens of the
    existing test the steps are 13 orders each."""
    n, tokens, heads = 1, 512, 2
    qkv = lazy_maximum_scores(tokens, order, n, heads)
    out = _h2_forms(ops, arm, qkv, n, tokens, heads)
    ref = _attention_ref(qkv, n, tokens, heads)
    e32 = _err(ops.attn_self(qkv, n, tokens, heads), ref)
    rise = _largest_rise_over_the_row_maximum(qkv, n, tokens, heads)
    print(f"{order}: largest rise of a block over its row's maximum {rise:.1f} binary orders; range flags {[out[p][2] for p in (0, 1, 2)]}")
    for pipe, (y, _, flagged) in out.items():
        assert bool(torch.isfinite(y).all())
        if pipe == 2 and flagged:
            assert rise > 92 - 7, f"the lazy loop raised its range flag at a rise of {rise:.1f} binary orders"
            continue
        assert flagged == 0
        _f16x2_class(e32, _err(y, ref), 2e-6)
    assert order == "steps" or out[2][2] == 0
    assert torch.equal(out[1][0], out[0][0]) and torch.equal(out[1][1], out[0][1])


@pytest.mark.parametrize("n,heads,tokens", [(3, 5, 256), (1, 3, 2048), (1, 3, 2304)])
def test_attention_workgroup_order(ops, arm, n, heads, tokens):
    """LDMK_ATTN_XCD=0 (launch order instead of the re-deal over the XCDs): 30 and 27 workgroups -- no multiples of 8, so the
    re-deal's ragged last round is in play -- and 24 (2048 tokens: 8 query tiles x 3 heads)."""
    gx = -(-tokens // 256) if tokens >= 2048 else -(-tokens // 128)
    assert gx * heads * n == {256: 30, 2048: 24, 2304: 27}[tokens]
    qkv = (1.5 * rnd(550, n * tokens, 3 * heads * 32)).cuda()
    flag = _flag()
    y, = _run_both(arm, "LDMK_ATTN_XCD", 0, lambda: (ops.attn_self(qkv, n, tokens, heads, h2_flag=flag),))
    ref = _attention_ref(qkv, n, tokens, heads)
    _f16x2_class(_err(ops.attn_self(qkv, n, tokens, heads), ref), _err(y, ref), 2e-6)
    assert int(flag.item()) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# LDMK_WGRAD_TR, LDMK_WINO_STAGED
def test_bf16_weight_gradient_with_the_strided_gather(ops, arm):
    """LDMK_WGRAD_TR=0: wgrad_kernel<BF = true> instead of wgrad_tr_kernel.  The integer cases of test_wgrad_rows_exact,
    test_wgrad_batched_split_exact and test_wgrad_conv_exact in bf16 compute: the float64 result exactly, sentinels intact -- what
    those tests demand of the default arm, hence the same bits there; on random operands dW is bit-equal and the fused bias
    gradient (summed in another order) keeps its tolerance, which is the switch's contract."""
    import test_backward_edges_gpu as E
    with arm("LDMK_WGRAD_TR", 0), torch.enable_grad():
        for R, Kw, N in E.WGRAD_ROWS:
            E.test_wgrad_rows_exact(ops, R, Kw, N, "bf16")
        E.test_wgrad_batched_split_exact(ops, "bf16")
        for case in E.CONV_CASES:
            E.test_wgrad_conv_exact(ops, case, "bf16")
    # and on operands that are not integers
    from dsml_thesis_amd import train_ops as T
    R, Kw, N = 2049, 288, 160
    a, dy = rnd(960, R, Kw).cuda(), rnd(961, R, N).cuda()

    def launch():
        T.set_compute("bf16")
        try:
            dw, db = torch.zeros(Kw, N, device="cuda"), torch.zeros(N, device="cuda")
            E._launch_wgrad(T, R, Kw, N, a, dy, dw, splitr=3, dbias=db)
        finally:
            T.set_compute("f32")
        return dw, db
    with arm("LDMK_WGRAD_TR", None):
        dw, db = launch()
    with arm("LDMK_WGRAD_TR", 0):
        dw0, db0 = launch()
    assert torch.equal(dw0, dw), "dW: the same products in the same order"
    # (the fused bias gradient is an fp32 column sum of dY that each kernel forms in its own order: the bound of test_bf16_gpu.test_bf16_wgrad)
    for got in (db, db0):
        close(got, dy.cpu().double().sum(0).float(), 1e-5, 1e-4)
    close(dw0, (a.cpu().to(torch.bfloat16).double().t() @ dy.cpu().to(torch.bfloat16).double()).float(), 5e-5, 5e-4)   # (test_bf16_gpu.test_bf16_wgrad)


@pytest.mark.parametrize("case", [WINOGRAD_CASES[0], WINOGRAD_CASES[3]])
def test_winograd_first_transforms(ops, arm, case):
    """LDMK_WINO_STAGED=0: the public Winograd transforms on their first kernels.  Two cases of
    test_conv3x3_winograd_matches_conv2d through ops.conv3x3_winograd (result and GroupNorm records), and the pre-split input
    transforms of both arithmetics on the same geometry: the default arm's bits."""
    from dsml_thesis_amd import lib as L
    refs = []

    def conv():
        y, part, ref = winograd_case(ops, case)
        refs.append(ref)
        return y, part
    y, part = _run_both(arm, "LDMK_WINO_STAGED", 0, conv)
    assert part is not None
    close(nchw(y), refs[0].float(), 1e-4, 1e-4)
    n, h, w_, c0, c1, _, pro, _ = case
    x0 = rnd(970, n, h, w_, c0).cuda()
    x1 = rnd(971, n, h, w_, c1).cuda() if c1 else None
    coef = torch.stack([1.0 + 0.2 * rnd(972, n, c0 + c1), 0.3 * rnd(973, n, c0 + c1)], 1).contiguous().cuda()
    tiles, flag = n * (h // 2) * (w_ // 2), _flag()

    def inputs():
        v3, vh = ops.ps_empty(tiles, c0 + c1, batch=16), ops.ps_empty(tiles, c0 + c1, batch=16, h2=True)
        v3.zero_(), vh.zero_()
        args = (x0.data_ptr(), c0, 0 if x1 is None else x1.data_ptr(), c1, coef.data_ptr(), 1, n, h, w_)
        L.call("ldmk_winograd_input_ps", *args, v3.data_ptr(), ops.stream())
        L.call("ldmk_winograd_input_ps_h2", *args, vh.data_ptr(), flag.data_ptr(), ops.stream())
        return v3, vh
    _run_both(arm, "LDMK_WINO_STAGED", 0, inputs)
    assert int(flag.item()) == 0
