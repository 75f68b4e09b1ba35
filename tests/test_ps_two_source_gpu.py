"""The pre-split GEMM tile with TWO A sources (csrc/igemm_ps.hip, ldmk_igemm_args.a_ps1 / a_ps_k0): columns [0, a_ps_k0) of A are
one PS tensor, columns [a_ps_k0, K) another -- the K-concat [A0 | A1] without a tensor that holds it.  The bar is the kernel's
contract: the products, their order and the split-K partition are those of the single-source launch on pack([A0 | A1]), so the
results are BITWISE equal at equal (tile_cfg, splitk), GroupNorm records included.  And the host-side refusals (ldmk_igemm_check:
no kernel runs)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rnd
from test_ops_gpu import ops  # noqa: F401  (the `ops` fixture)

pytestmark = pytest.mark.gpu

NS = (64, 160, 320)
SPLITS = (1, 2, 3)
# M = 96 / 288 with GroupNorm records (rows_per_sample 32: the lane = column epilogue), M = 80 without (the transposed epilogue; the
# last 32-row block is padding and the 128 / 256-row tiles have an edge)
MS = ((96, True), (288, True), (80, False))


def _launch(ops, M, N, K, wp, wps, a_ps, bias, res, cfg, sk, ws, flag, records, a_ps1=None, k0=0):
    out = torch.full((M, N), float("nan"), device="cuda")
    a = ops.make_igemm_args(M, N, K, None, K, wp, out, N, 32 if records else M, tile_cfg=cfg, splitk=sk, splitk_ws=ws, a_ps=a_ps, w_ps=wps,
                            bias=bias, residual=res, range_flag=flag, a_ps1=a_ps1, a_ps_k0=k0)
    rec = None
    if records:
        rec = torch.full((M // 32, N, 3), float("nan"), device="cuda")
        a.stats_out = rec.data_ptr()
    ops.igemm(a)
    return out, rec


@pytest.mark.parametrize("cfg", [23, 24, 27])
@pytest.mark.parametrize("K0,K1", [(128, 32), (640, 160)])
@pytest.mark.parametrize("h2", [False, True], ids=["bf16x3", "f16x2"])
def test_two_source_launch_is_bitwise_the_single_source_launch_on_the_concat(ops, h2, K0, K1, cfg):
    """K = 800 is 25 chunks of 32: splitk 2 (13 + 12) and 3 (9 + 9 + 7) both put the source boundary (chunk 20) inside a slice; at
    K = 160 splitk 2 (3 + 2 chunks) puts it (chunk 4) in the last slice.  N = 64 / 160 / 320 against tiles 160 and 320 wide: column
    edges and more than one column tile."""
    K = K0 + K1
    flag = torch.zeros(1, dtype=torch.int32, device="cuda") if h2 else None
    for N in NS:
        wp = (rnd(801, K, N) / np.sqrt(K)).cuda().contiguous()
        wps = ops.pack_wps(wp, h2=h2)
        bias = (0.1 * rnd(802, N)).cuda()
        for M, records in MS:
            a0, a1 = rnd(803, M, K0).cuda(), rnd(804, M, K1).cuda()
            res = rnd(805, M, N).cuda()
            p0, p1 = ops.pack_ps(a0, h2_flag=flag), ops.pack_ps(a1, h2_flag=flag)
            pc = ops.pack_ps(torch.cat([a0, a1], 1).contiguous(), h2_flag=flag)
            ws = torch.empty(3 * M * N, device="cuda")
            for sk in SPLITS:
                two, rec2 = _launch(ops, M, N, K, wp, wps, p0, bias, res, cfg, sk, ws, flag, records, a_ps1=p1, k0=K0)
                one, rec1 = _launch(ops, M, N, K, wp, wps, pc, bias, res, cfg, sk, ws, flag, records)
                what = (h2, K0, K1, cfg, N, M, sk)
                assert torch.isfinite(one).all(), what
                assert torch.equal(two, one), what
                if records:
                    assert torch.isfinite(rec1).all() and torch.equal(rec2, rec1), what
            if N == 160 and M == 288:      # (the single-source launch itself against float64, once per case)
                ref = torch.cat([a0, a1], 1).double().cpu() @ wp.double().cpu() + bias.double().cpu() + res.double().cpu()
                assert (one.double().cpu() - ref).abs().max().item() < 2e-5
    if h2:
        assert flag.item() == 0


def test_two_source_refusals_on_the_host(ops):
    """What csrc/igemm_ps.hip refuses for a_ps1, reported by ldmk_igemm_check without a launch."""
    from dsml_thesis_amd import lib as L
    lib = L.load()
    M, K0, K1, N = 128, 128, 64, 128
    K = K0 + K1
    wp = (rnd(811, K, N) / 12).cuda().contiguous()
    wps = ops.pack_wps(wp)
    p0, p1 = ops.pack_ps(rnd(812, M, K0).cuda()), ops.pack_ps(rnd(813, M, K1).cuda())
    out = torch.empty(M, N, device="cuda")

    def args(cfg=23, k0=K0, **kw):
        return ops.make_igemm_args(M, N, K, None, K, wp, out, N, M, tile_cfg=cfg, splitk=1, a_ps=p0, w_ps=wps, a_ps1=p1, a_ps_k0=k0, **kw)

    def refused(a, word=b"a_ps1"):
        return lib.ldmk_igemm_check(ctypes.byref(a)) != 0 and word in lib.ldmk_last_error()

    assert lib.ldmk_igemm_check(ctypes.byref(args())) == 0
    for k0 in (0, K, K0 + 16, 16, -32):                                   # both widths positive multiples of 32
        assert refused(args(k0=k0)), k0
    assert refused(args(cfg=29)) and refused(args(cfg=30))                # the warp-specialised tiles
    a = args()
    a.batch, a.a_ps_bstride, a.w_ps_bstride, a.out_bstride = 2, 1, 1, M * N
    assert refused(a)
    st, cs = torch.zeros(M, 2, device="cuda"), torch.zeros(N, device="cuda")
    assert refused(args(tf=L.TF_LAYERNORM_FOLDED, row_stats=st, ln_colsum=cs))
    assert refused(args(epi=L.EPI_GEGLU, cfg=25))
    # the fused QKV projection (F16X2 only) and the conv-mode tile
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    w3 = (rnd(814, K, 96) / 12).cuda().contiguous()
    kv = torch.empty(lib.ldmk_attn_kv_split_h2_bytes(2, 64, 1), device="cuda", dtype=torch.uint8)
    o3 = torch.empty(M, 96, device="cuda")
    a = ops.make_igemm_args(M, 96, K, None, K, w3, o3, 96, 64, tile_cfg=23, splitk=1, a_ps=p0, w_ps=ops.pack_wps(w3, h2=True), range_flag=flag,
                            attn_kv=(kv, 64, 1), a_ps1=p1, a_ps_k0=K0)
    assert refused(a)
    a.a_ps1 = None
    assert lib.ldmk_igemm_check(ctypes.byref(a)) == 0                      # (the same launch with one source is legal)
    wc = (rnd(815, 9 * 32, 32) / 12).cuda().contiguous()
    oc = torch.empty(2 * 64, 32, device="cuda")
    a = ops.make_igemm_args(128, 32, 9 * 32, None, 32, wc, oc, 32, 64, conv=(8, 8, 8, 8, 1, 1, 0), tile_cfg=27, splitk=1, a_ps=p0,
                            w_ps=ops.pack_wps(wc, h2=True), range_flag=flag, a_ps1=p1, a_ps_k0=32)
    assert refused(a)
    a.a_ps1 = None
    assert lib.ldmk_igemm_check(ctypes.byref(a)) == 0
    # a tile that does not read the PS layout at all
    a = args(cfg=5)
    assert lib.ldmk_igemm_check(ctypes.byref(a)) != 0
