"""GPU: exact-arithmetic and guard-memory tests of the forward implicit GEMM, ldmk_igemm (csrc/igemm.hip, igemm_ps.hip, igemm_ws.hip,
rgemm.hip, sgemm.hip and the shared epilogue ldmk_epilogue.h): all 33 pinned tile configurations, the four arithmetics, both gather
paths, both split-K forms.

Exact tests.  Operands are integers in [-2, 2] (affine prologue: scale in {1, 2, -1}, integer shift), bias / per-sample vector /
residual integers in [-5, 5], alpha in {1, 0.5}, K <= 9 * 96: every product and partial sum is an integer (or half-integer) far
below 2^24 and every operand is exact in bf16 and in scaled fp16 (the F16X2 scales are powers of two), so the result must equal the
float64 reference of tests/igemm_ref.py BITWISE in every arithmetic -- one wrong row, column, tap, K chunk or slab shows.

Guards.  Every launch writes into memory prefilled with SENT: ldc = N + 12, 32 spare rows behind row M (they are also the gap between
batch entries), a tail behind the split-K scratch (sized by ldmk_igemm_workspace_elems), behind stats_out, the counters and the
range flag.  Inputs are surrounded by ALLOCATED NaN rows (before and after each source, between batch entries, in the weight columns
N .. ldb - 1, around the residual): a mis-addressed read shows as a NaN or a wrong value, it does not fault.

Support table.  expected() mirrors rgemm_unsupported, sgemm_unsupported, igemm_ws_unsupported, igemm_ps_unsupported and the checks of
igemm_entry.  For every case ldmk_igemm_check is asked about all 33 tiles x 6 operand modes and must agree with the table in both
directions; every pair the table admits is launched.  Nothing is skipped because check refused it."""
import ctypes
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import igemm_ref as R
from conftest import rnd
from test_backward_edges_gpu import SENT, _exact, _ints
from test_ops_gpu import nhwc, ops  # noqa: F401  (the `ops` fixture)

pytestmark = pytest.mark.gpu

NAN = float("nan")
ISENT = -7                      # sentinel of the integer guards (counters, range flag)
PADR = 3                        # NaN rows before and after every A source
# tile_cfg -> (BM, BN) and what else the host rules read
LDS = {1: (128, 128), 2: (64, 128), 3: (64, 64), 4: (64, 64), 5: (128, 160), 6: (64, 160)}
ROW = {7: (1, 5), 8: (2, 5), 9: (1, 4), 10: (2, 4), 11: (1, 2), 12: (1, 1)}                                   # (tm, tn) in 32s
SLAB = {13: (2, 1, 4), 14: (2, 2, 4), 15: (1, 1, 4), 16: (1, 2, 4), 17: (1, 1, 8), 18: (1, 1, 16), 19: (2, 1, 8), 20: (1, 2, 8)}   # (tm, tn, waves)
WS = {21: (256, 160), 22: (256, 128)}
PS = {23: (256, 160), 24: (256, 320), 25: (256, 256), 26: (128, 320), 27: (128, 160), 28: (128, 256), 29: (256, 160), 30: (256, 128),
      31: (256, 160), 32: (256, 128), 33: (128, 256)}
PS_EVEN_TN = (25, 28, 30, 32, 33)
PS_CONV = (23, 24, 26, 27)
ALL_CFG = range(1, 34)
# operand modes: arithmetic + the form the operands are passed in
MODES = {"f32": 0, "bf16": 1, "bf16i": 1, "x3": 2, "x3a": 2, "h2": 3}       # bf16i: ldmk_pack_wbf16t image; x3a: a_split as well
TF_NONE, TF_AFFINE, TF_SILU, TF_LN, TF_LNF = 0, 1, 2, 3, 4


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_error():
    """A sticky HIP error (an illegal access is one) ends the session: nothing more is launched on a device that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error during this test, nothing more is launched: {e}", returncode=3)


def family(cfg):
    return "lds" if cfg <= 6 else "row" if cfg <= 12 else "slab" if cfg <= 20 else "ws" if cfg <= 22 else "ps"


def tile(cfg):
    """(BM, BN) of a tile_cfg"""
    if cfg in LDS:
        return LDS[cfg]
    if cfg in ROW:
        return 32 * ROW[cfg][0], 32 * ROW[cfg][1]
    if cfg in SLAB:
        return 32 * SLAB[cfg][0], 32 * SLAB[cfg][1]
    return WS[cfg] if cfg in WS else PS[cfg]


def prob(M=None, N=32, K=None, c0=32, c1=0, conv=None, n=1, rps=None, **kw):
    """A problem.  conv = (h, w, stride, pad_lo, upsample) with n samples; rows mode otherwise (rps = rows per sample)."""
    p = SimpleNamespace(N=N, c0=c0, c1=c1, n=n, b_trans=False, batch=1, alpha=1.0, bias=True, vec=False, res=True, tf=TF_NONE,
                        splitk=1, counters=False, raw=False, skip=None, geglu=False, stats=False, out_ps=False, seed=1000, big=None)
    p.__dict__.update(kw)
    if conv is not None:
        h, w, stride, pad_lo, ups = conv
        oh, ow = R.out_size(h, stride, pad_lo, ups), R.out_size(w, stride, pad_lo, ups)
        p.conv = (h, w, oh, ow, stride, pad_lo, ups)
        p.rps, p.M = oh * ow, n * oh * ow
        p.K = 9 * (c0 + c1) + (sum(p.skip) if p.skip else 0)
    else:
        p.conv, p.M, p.K = None, M, c0 + c1
        p.rps = rps or M
        p.n = -(-M // p.rps)
    assert K is None or K == p.K
    return p


# ---------------------------------------------------------------------------------------------------------------------------
# the support table: which (tile_cfg, mode) pairs run a problem -- the rules of the four *_unsupported functions and igemm_entry
def expected(p, cfg, mode):
    comp, fam, conv = MODES[mode], family(cfg), p.conv is not None
    ups = p.conv[6] if conv else 0
    sk = p.splitk
    fast = (ups == 0 or (ups == 1 and p.c1 == 0)) and (p.batch <= 1 or p.c1 == 0)          # igemm_fast_gather_ok
    # ---- igemm_entry
    if p.skip and not (conv and fam == "slab"):
        return False
    if p.N % 4 or (conv and p.batch > 1):
        return False
    if p.tf == TF_LN and conv:
        return False
    if p.tf == TF_LNF and (conv or p.stats or p.batch > 1):
        return False
    if p.geglu and (p.N % 64 or p.res or p.vec):
        return False
    if p.stats and (p.M % 32 or p.rps % 32 or p.geglu or p.batch > 1):
        return False
    if comp == 2 and fam != "ps" and (p.b_trans or not fast):
        return False
    if comp == 3 and (fam not in ("lds", "ps") or (fam == "lds" and (p.b_trans or not fast))):
        return False
    if mode == "bf16i" and (p.b_trans or p.batch > 1):
        return False
    if mode == "x3a" and (conv or p.c1 or p.batch > 1 or p.tf not in (TF_NONE, TF_LNF) or fam != "lds"):
        return False
    if comp != 0 and fam in ("row", "slab"):
        return False
    if fam == "lds":
        if p.raw and (sk < 2 or p.batch > 1 or p.counters or p.stats):
            return False
        return True
    if fam == "row":                                                                       # rgemm_unsupported (K is never split)
        tm, tn = ROW[cfg]
        if conv or p.b_trans or p.batch > 1 or p.tf == TF_SILU or p.N % (32 * tn):
            return False
        if p.geglu and tn % 2:
            return False
        return not ((p.tf == TF_AFFINE or p.vec) and p.rps % (32 * tm))
    if fam == "slab":                                                                      # sgemm_unsupported
        tm, tn, nw = SLAB[cfg]
        if p.b_trans or p.batch > 1 or p.tf in (TF_SILU, TF_LN) or p.N % (32 * tn):
            return False
        if conv and (p.conv[4] != 1 or ups or p.conv[5] != 1 or p.c1 or p.tf != TF_NONE):
            return False
        if p.geglu and (tn % 2 or (sk > 1 and not p.raw)):
            return False
        if (p.tf == TF_AFFINE or p.vec) and p.rps % (32 * tm):
            return False
        if nw * sk > p.K // 8 or (sk > 1 and p.counters) or (p.raw and sk < 2):
            return False
        return True
    if fam == "ws":                                                                        # igemm_ws_unsupported
        if mode != "x3" or p.b_trans or ups or p.counters or p.skip:
            return False
        if p.geglu and (cfg != 22 or sk > 1):
            return False
        return sk <= p.K // 32 and not (p.raw and sk < 2)
    # ---- igemm_ps_unsupported
    if mode not in ("x3", "h2") or (mode == "h2" and cfg in (29, 30)):
        return False
    if conv:
        if mode != "h2" or cfg not in PS_CONV or p.c1 or ups or p.tf != TF_NONE or p.out_ps or p.batch > 1 or p.geglu:
            return False
        if (p.c0 // 32) % sk:
            return False
    if p.b_trans or ups or p.skip or p.counters or p.tf not in (TF_NONE, TF_LNF) or p.K % 32 or p.N % 32:
        return False
    if p.geglu and (cfg not in PS_EVEN_TN or sk > 1):
        return False
    if sk > p.K // 32 or (p.raw and sk < 2):
        return False
    if p.out_ps and (sk > 1 or p.batch > 1 or p.stats):
        return False
    return True


# ---------------------------------------------------------------------------------------------------------------------------
# data, reference and device operands of a problem (made once per problem)
def _scale_shift(seed, n, C):
    return torch.stack([torch.tensor([1.0, 2.0, -1.0])[_ints(seed, n, C, lo=0, hi=2).long()], _ints(seed + 1, n, C, lo=-3, hi=3)], 1).contiguous()


def data(p):
    if hasattr(p, "d"):
        return p.d
    d = SimpleNamespace()
    s, B, conv = p.seed, p.batch, p.conv is not None
    shp = (p.n, p.conv[0], p.conv[1]) if conv else (p.M,)
    d.x0 = _ints(s, B, *shp, p.c0)
    if p.big is not None:                                   # one activation outside the F16X2 range (never compared: flag test)
        d.x0.view(-1)[p.big] = 1000.0
    d.x1 = _ints(s + 1, *shp, p.c1) if p.c1 else None       # (a batch offsets a0 and w only: one a1 for all entries)
    d.w = _ints(s + 2, B, p.K, p.N)
    d.bias = _ints(s + 3, p.N, lo=-5, hi=5) if p.bias else None
    d.vec = _ints(s + 4, p.n, p.N, lo=-5, hi=5) if p.vec else None
    d.res = _ints(s + 5, B, p.M, p.N, lo=-5, hi=5) if p.res else None
    d.coef = _scale_shift(s + 6, p.n, p.c0 + p.c1) if p.tf == TF_AFFINE else None
    d.skip0 = _ints(s + 8, p.M, p.skip[0]) if p.skip else None
    d.skip1 = _ints(s + 9, p.M, p.skip[1]) if p.skip and p.skip[1] else None
    d.A, refs = [], []
    for b in range(B):
        sk = None if not p.skip else (d.skip0 if d.skip1 is None else torch.cat([d.skip0, d.skip1], 1))
        A = R.operand_matrix(d.x0[b], d.x1, coef=d.coef, conv=p.conv[4:] if conv else None, rows_per_sample=p.rps, skip=sk)
        assert A.shape == (p.M, p.K)
        d.A.append(A)
        refs.append(R.igemm_ref(A, d.w[b], p.alpha, d.bias, d.vec, p.rps, None if d.res is None else d.res[b]))
    d.ref = torch.stack(refs)                               # [batch][M][N] float64
    p.d = d
    return d


def _padded(x, pad_rows):
    """[B][rows][c] -> cuda buffer [B][pad + rows + pad][c] with NaN padding rows; returns (buffer, pointer of row 0 of entry 0, batch stride)"""
    B, rows, c = x.shape
    buf = torch.full((B, rows + 2 * pad_rows, c), NAN)
    buf[:, pad_rows:pad_rows + rows] = x
    buf = buf.cuda()
    return buf, buf.data_ptr() + 4 * pad_rows * c, (rows + 2 * pad_rows) * c


def dev(ops, p):
    if hasattr(p, "g"):
        return p.g
    d, g = data(p), SimpleNamespace()
    B, conv = p.batch, p.conv is not None
    g.a0buf, g.a0, g.a_bstride = _padded(d.x0.reshape(B, -1, p.c0), PADR)
    g.a1buf, g.a1 = (None, 0) if d.x1 is None else _padded(d.x1.reshape(1, -1, p.c1), PADR)[:2]
    # fp32 weights as the F32 / BF16 forms read them: leading dimension with NaN columns, a NaN gap between batch entries
    wsrc = d.w.transpose(1, 2) if p.b_trans else d.w                      # b_trans: [N][ldb] (torch [out][in])
    g.ldb = wsrc.shape[2] + 4
    wl = torch.full((B, wsrc.shape[1] * g.ldb + 8), NAN)
    wl[:, :wsrc.shape[1] * g.ldb].view(B, wsrc.shape[1], g.ldb)[:, :, :wsrc.shape[2]] = wsrc
    g.wl, g.wl_bstride = wl.cuda(), wl.shape[1]
    # contiguous [K][N] weights and their images (the 16-bit arithmetics, the fragment-order copy, the PS layout)
    g.wc = d.w.cuda().contiguous() if B > 1 else d.w[0].cuda().contiguous()
    if not p.b_trans:
        ops.pack_wsplit(g.wc, batch=B)
        ops.pack_wsplit_h2(g.wc, batch=B)
        g.wbf16t = ops.pack_wbf16t(g.wc) if B == 1 else None
        g.wfrag = ops.pack_wfrag(g.wc) if B == 1 and p.N % 32 == 0 else None
        g.flag0 = torch.zeros(1, dtype=torch.int32, device="cuda")
        if p.K % 16 == 0:
            g.wps, g.wps_h2 = ops.pack_wps(g.wc, batch=B), ops.pack_wps(g.wc, batch=B, h2=True)
            if conv:                                                     # the stored activation [n h w][c0]; a second source is not taken
                act = d.x0[0].reshape(-1, p.c0).cuda().contiguous()
            else:
                act = torch.stack([a.float() for a in d.A]).cuda().contiguous() if B > 1 else d.A[0].float().cuda().contiguous()
            g.aps, g.aps_h2 = ops.pack_ps(act), ops.pack_ps(act, h2_flag=g.flag0)
    if not conv and not p.c1 and B == 1:
        g.a_split = torch.stack(R.split3(d.x0[0])).cuda().contiguous()    # [3][M][K] bf16
    g.bias = None if d.bias is None else d.bias.cuda()
    g.vec = None if d.vec is None else d.vec.cuda()
    g.coef = None if d.coef is None else d.coef.cuda()
    g.skip0 = None if d.skip0 is None else _padded(d.skip0[None], PADR)
    g.skip1 = None if d.skip1 is None else _padded(d.skip1[None], PADR)
    p.g = g
    return g


def desc(p):
    return {k: v for k, v in vars(p).items() if k not in ("d", "g")}


def ncols(p):
    return p.N // 2 if p.geglu else p.N


def make(ops, p, cfg, mode, extra=None):
    """ldmk_igemm_args of problem p on (tile_cfg, mode) with fresh guarded outputs; returns (args, buffers)."""
    from dsml_thesis_amd import lib as L
    d, g = data(p), dev(ops, p)
    comp, fam, conv, B = MODES[mode], family(cfg), p.conv is not None, p.batch
    o = SimpleNamespace()
    nc = ncols(p)
    o.ldc = nc + (16 if p.out_ps else 12)
    o.out = torch.full((B, p.M + 32, o.ldc), SENT, device="cuda")
    o.res = None
    if d.res is not None:                                       # (read-only: one NaN-framed copy per problem)
        if not hasattr(g, "res"):
            rb = torch.full((B, p.M + 32, o.ldc), NAN)
            rb[:, :p.M, :p.N] = d.res
            g.res = rb.cuda()
        o.res = g.res
    packed = not p.b_trans and (fam != "lds" or mode not in ("f32", "bf16"))
    w, ldb, w_bstride = (g.wc, p.N, p.K * p.N) if packed else (g.wl, g.ldb, g.wl_bstride)
    kw = dict(extra or {})
    ps = fam == "ps" and hasattr(g, "wps")
    if ps:
        h2 = mode == "h2"
        kw.update(a_ps=g.aps_h2 if h2 else g.aps, w_ps=g.wps_h2 if h2 else g.wps)
        if p.out_ps:
            o.ops_bytes = L.load().ldmk_ps_bytes_h2(p.M, o.ldc) if h2 else L.load().ldmk_ps_bytes(p.M, o.ldc)
            o.out_ps = torch.full((o.ops_bytes + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
            kw.update(out_ps=o.out_ps)
    rows_ps = ps and not conv                                   # rows mode on a pre-split tile: A = pack_ps of the concat, c0 = K
    a = ops.make_igemm_args(p.M, p.N, p.K, None if ps else g.a0, p.K if rows_ps else p.c0, w, o.out, o.ldc, p.rps,
                            a1=None if rows_ps or not p.c1 else g.a1, c1=0 if rows_ps else p.c1,
                            conv=p.conv, tf=p.tf, tf_coef=g.coef, b_trans=p.b_trans, ldb=ldb, bias=g.bias, batch_vec=g.vec,
                            batch_vec_ld=p.N if g.vec is not None else 0, residual=o.res, epi=1 if p.geglu else 0, batch=B,
                            a_bstride=g.a_bstride if B > 1 else 0, w_bstride=w_bstride if B > 1 else 0,
                            out_bstride=(p.M + 32) * o.ldc if B > 1 else 0, alpha=p.alpha, splitk=p.splitk,
                            w_frag=g.wfrag if fam in ("row", "slab") and not p.b_trans else None, tile_cfg=cfg, raw_slabs=p.raw, **kw)
    if p.skip:
        a.K = p.K
        a.skip_a0, a.skip_c0 = g.skip0[1], p.skip[0]
        a.skip_a1, a.skip_c1 = (g.skip1[1], p.skip[1]) if g.skip1 is not None else (0, 0)
    # the arithmetic and the operand forms of `mode` (set by hand: make_igemm_args refuses combinations the table must see refused)
    o.flag = torch.tensor([0, ISENT, ISENT, ISENT], dtype=torch.int32, device="cuda")
    a.compute = comp
    if comp == 3:
        a.range_flag = o.flag.data_ptr()
    if not ps and packed and comp >= 2:
        ops.attach_image(a, ops.split_of(w.data_ptr()) if comp == 2 else ops.split_h2_of(w.data_ptr()), o.flag)
    if mode == "bf16i":                                        # (no image exists under b_trans / batching: any non-null pointer is refused)
        img = getattr(g, "wbf16t", None)
        a.w_split, a.w_split_ld = (img.data_ptr(), img.shape[-1]) if img is not None else (g.wl.data_ptr(), (p.K + 7) // 8 * 8)
    if mode == "x3a" and hasattr(g, "a_split"):
        a.a_split, a.a_split_ld = g.a_split.data_ptr(), g.a_split.shape[-1]
    if mode == "x3a" and not hasattr(g, "a_split"):             # (no pre-split A exists for this problem: any non-null pointer is refused)
        a.a_split, a.a_split_ld = g.a0, p.K
    # guarded scratch
    o.need = max(0, L.load().ldmk_igemm_workspace_elems(ctypes.byref(a)))
    if p.splitk > 1:
        o.ws = torch.full((o.need + 1024,), SENT, device="cuda")
        a.splitk_ws, a.splitk_ws_elems = o.ws.data_ptr(), o.need
    if p.counters:
        o.ntile = B * -(-p.M // 64) * -(-p.N // 64)
        o.cnt = torch.zeros(o.ntile + 64, dtype=torch.int32, device="cuda")
        o.cnt[o.ntile:] = ISENT
        a.splitk_counters, a.splitk_counters_len = o.cnt.data_ptr(), o.ntile
    if p.stats:
        o.nrec = (p.M // 32) * p.N * 3
        o.stats = torch.full((o.nrec + 96,), SENT, device="cuda")
        a.stats_out = o.stats.data_ptr()
    return a, o


def check(a):
    from dsml_thesis_amd import lib as L
    return L.load().ldmk_igemm_check(ctypes.byref(a)) == 0


def guards(p, o, what):
    """everything outside the result still holds its sentinel; the counters are zero again"""
    out = o.out.cpu()
    nc = ncols(p)
    if p.raw:
        assert (out == SENT).all(), f"{what}: raw_slabs must not write `out`"
    else:
        assert (out[:, :p.M, nc:] == SENT).all(), f"{what}: columns N..ldc-1 were written"
    assert (out[:, p.M:] == SENT).all(), f"{what}: rows past M (the gap between batch entries) were written"
    if p.splitk > 1:
        assert (o.ws[o.need:] == SENT).all(), f"{what}: the split-K scratch was written past splitk*M*N"
    if p.counters:
        assert int(o.cnt[:o.ntile].abs().sum()) == 0, f"{what}: the arrival counters are not zero again"
        assert (o.cnt[o.ntile:] == ISENT).all(), f"{what}: counters past the tile count were written"
    if p.stats:
        assert (o.stats[o.nrec:] == SENT).all(), f"{what}: stats_out was written past M/32 tiles"
    assert (o.flag[1:] == ISENT).all(), f"{what}: memory behind the range flag was written"
    return out


def launch_exact(ops, p, cfg, mode, extra=None):
    """run, compare bitwise with the float64 reference, check every guard; returns the [batch][M][N] result (raw_slabs: the slabs)"""
    what = f"tile_cfg={cfg} {mode} M={p.M} N={p.N} K={p.K} splitk={p.splitk}"
    d = data(p)
    a, o = make(ops, p, cfg, mode, extra)
    ops.igemm(a)
    out = guards(p, o, what)
    if MODES[mode] == 3:
        assert int(o.flag[0]) == 0, f"{what}: range_flag raised on in-range data"
    if p.raw:
        slabs = o.ws[:o.need].cpu().view(p.splitk, p.M, p.N)
        scale = 2.0 ** -(ops.F16X2_A_EXP + (a.w_scale_exp if MODES[mode] == 3 else -ops.F16X2_A_EXP))
        got = (slabs.sum(0) * scale * p.alpha + (0 if d.bias is None else d.bias) + (0 if d.res is None else d.res[0]))[None]
        if d.vec is not None:
            got = got + d.vec[torch.arange(p.M) // p.rps]
    else:
        got = out[:, :p.M, :p.N]
    _exact(got, d.ref, what)
    return got


def sweep(ops, p, run_on, modes_run=None):
    """ldmk_igemm_check against the table for all 33 tiles x 6 modes; every admitted pair among `run_on` tiles is launched.
    Returns {(cfg, mode): result}."""
    ran = {}
    for cfg in ALL_CFG:
        for mode in MODES:
            want = expected(p, cfg, mode)
            a, _ = make(ops, p, cfg, mode)
            got = check(a)
            assert got == want, (f"ldmk_igemm_check {'admits' if got else 'refuses'} tile_cfg={cfg} {mode}, the support table says "
                                 f"{'runs' if want else 'refused'}: {desc(p)}")
            if want and cfg in run_on and (modes_run is None or mode in modes_run):
                ran[(cfg, mode)] = launch_exact(ops, p, cfg, mode)
    return ran


# ---------------------------------------------------------------------------------------------------------------------------
# 1. rows mode
def rows_cases(cfg):
    """The rows-mode problems of one tile: M in {1, 33, BM + 1}, K in {32, 64, 96}; N = 4 / 36 / 132 on the LDS tiles, one tile's
    width and one tile plus 32 columns elsewhere; one / two sources, b_trans with ldb = K + 4, batches with gaps."""
    bm, bn = tile(cfg)
    ns = (4, 36, 132) if cfg in LDS else (bn, bn + 32)
    ms = (1, 33, bm + 1)
    # a slab tile gives each of its waves at least one 8-deep K block: the 8-wave tiles need K >= 64, the 16-wave tile 18 K >= 128
    # (the smaller K stay in the list: refused there).  Three K run on every tile.
    nw = SLAB[cfg][2] if cfg in SLAB else 4
    ks = (32, 64, 96) + {4: (), 8: (128,), 16: (128, 160, 192)}[nw]
    k_lo, k_hi, c1 = max(32, 8 * nw), max(96, 8 * nw + 32), max(64, 8 * nw - 32)
    cases = [prob(M=m, N=ns[0], c0=k) for m in ms for k in ks]
    cases += [prob(M=m, N=n_, c0=k) for n_ in ns[1:] for m, k in ((33, k_lo), (bm + 1, k_hi))]
    # two sources (c0 = 32, c1 = 64), alpha = 0.5, a per-sample vector whose samples (5 rows) straddle every 32-row tile
    cases += [prob(M=m, N=ns[-1], c0=32, c1=c1, alpha=0.5, vec=True, rps=5) for m in (33, bm + 1)]
    cases += [prob(M=bm + 1, N=ns[0], c0=32, c1=c1, alpha=0.5)]                       # (without the vector: the row / slab tiles too)
    cases += [prob(M=33, N=ns[0], c0=64, b_trans=True, alpha=0.5)]
    cases += [prob(M=33, N=ns[-1], c0=64, batch=3)]
    cases += [prob(M=33, N=ns[0], c0=32, c1=64, batch=2)]                             # batched + two sources: the general gather
    return cases


@pytest.mark.parametrize("cfg", list(ALL_CFG))
def test_rows_mode_exact(ops, cfg):
    ran = set()
    for p in rows_cases(cfg):
        got = sweep(ops, p, (cfg,))
        ran |= set(got)
        fam = family(cfg)
        if fam == "lds":                                     # every arithmetic and operand form on every LDS tile that takes it
            want = {m for m in MODES if expected(p, cfg, m)}
            assert {m for _, m in got} == want
            if not p.b_trans and p.batch == 1 and not p.c1:
                assert want == set(MODES), (desc(p), want)
            if p.b_trans or (p.batch > 1 and p.c1):
                assert want == {"f32", "bf16"}
    modes = {m for _, m in ran}
    assert modes == {"lds": set(MODES), "row": {"f32"}, "slab": {"f32"}, "ws": {"x3"}, "ps": {"x3"} if cfg in (29, 30) else {"x3", "h2"}}[family(cfg)]


def test_every_tile_runs_an_exact_rows_case():
    """The table itself (no launch): each of tile_cfg 1..33 admits at least one rows-mode case -- three M, three K -- and the
    arithmetics of its family; a check that refuses everything fails test_rows_mode_exact, it cannot empty it."""
    count = 0
    for cfg in ALL_CFG:
        cases = rows_cases(cfg)
        admitted = [(p, m) for p in cases for m in MODES if expected(p, cfg, m)]
        assert {p.M for p, _ in admitted} >= {1, 33, tile(cfg)[0] + 1} and len({p.K for p, _ in admitted}) >= 3, cfg
        count += bool(admitted)
    assert count == 33


# ---------------------------------------------------------------------------------------------------------------------------
# 2. split-K: reduce launch, in-launch counter combine, raw slabs
@pytest.mark.parametrize("cfg", [c for c in ALL_CFG if family(c) != "row"])
def test_split_k_exact(ops, cfg):
    """splitk in {2, K / 32} on K = 96 (every slice of the second is ONE 32-deep chunk, fewer than a ring holds) and M = 33 and
    BM + 1: the reduce launch, the counter combine (tile_cfg 1..6) and raw_slabs agree bitwise with each other and the reference;
    one slice more than there are chunks is refused on the ws and ps tiles."""
    bm, bn = tile(cfg)
    fam = family(cfg)
    N = 36 if fam == "lds" else bn
    for M in (33, bm + 1):
        for sk in (2, 3):
            base = dict(M=M, N=N, c0=32, c1=64, alpha=0.5, vec=fam in ("lds", "ws", "ps"), rps=5, splitk=sk)
            if fam == "slab":                                # (every wave of every slice needs an 8-deep block of K)
                base.update(c0=max(96, 8 * SLAB[cfg][2] * sk), c1=0)
            forms = [prob(**base), prob(**base, raw=True)] + ([prob(**base, counters=True)] if fam == "lds" else [])
            results = []
            for p in forms:
                got = sweep(ops, p, (cfg,))
                assert got, (cfg, desc(p))
                results.append(got)
            for other in results[1:]:
                for key in results[0]:
                    if key in other:
                        assert torch.equal(results[0][key], other[key]), f"split-K forms differ on {key}"
    if fam in ("ws", "ps"):
        p = prob(M=33, N=bn, c0=96, splitk=4)
        assert not any(expected(p, cfg, m) for m in MODES)
        sweep(ops, p, ())
        a, o = make(ops, p, cfg, "x3")
        from dsml_thesis_amd import lib as L
        with pytest.raises(L.LdmkError, match="more K slices"):
            ops.igemm(a)
        assert (o.out == SENT).all() and (o.ws == SENT).all(), "refused, but memory was written"


# ---------------------------------------------------------------------------------------------------------------------------
# 3. conv mode
CONV_TILES = [c for c in ALL_CFG if family(c) in ("lds", "slab", "ws") or c in PS_CONV]
IMAGES = [(1, 1), (1, 5), (5, 1), (3, 8), (5, 7)]


def conv_cases(cfg):
    fam = family(cfg)
    N = 36 if fam == "lds" else tile(cfg)[1]
    cases = []
    for h, w in IMAGES:                                      # rows_per_sample 1, 5, 5, 24, 35: sample boundaries inside a tile
        for n in (1, 3):
            # per-sample vector + integer affine prologue, two sources ...
            cases.append(prob(N=N, c0=32, c1=32, conv=(h, w, 1, 1, 0), n=n, vec=True, tf=TF_AFFINE, alpha=0.5 if n == 3 else 1.0))
            # ... and the plain one-source form every conv-capable tile takes
            cases.append(prob(N=N, c0=32 if n == 1 else 64, conv=(h, w, 1, 1, 0), n=n, vec=fam != "slab"))
    for h, w in ((5, 7), (6, 4)):                            # stride 2, both pads
        for pad_lo in (1, 0):
            cases.append(prob(N=N, c0=32, c1=64, conv=(h, w, 2, pad_lo, 0), n=2, vec=True, tf=TF_AFFINE))
            cases.append(prob(N=N, c0=32, conv=(h, w, 2, pad_lo, 0), n=2, vec=True))
    cases.append(prob(N=N, c0=64, conv=(3, 5, 1, 1, 1), n=2, vec=True, tf=TF_AFFINE))            # upsample, one source: fast gather
    cases.append(prob(N=N, c0=32, c1=32, conv=(3, 5, 1, 1, 1), n=2, vec=True, tf=TF_AFFINE))     # two sources: the general gather
    cases.append(prob(N=N, c0=32, conv=(1, 1, 1, 1, 1), n=3))
    return cases


@pytest.mark.parametrize("cfg", CONV_TILES)
def test_conv_mode_exact(ops, cfg):
    ran = set()
    for p in conv_cases(cfg):
        ran |= set(sweep(ops, p, (cfg,)))
    fam = family(cfg)
    assert {m for _, m in ran} == {"lds": set(MODES) - {"x3a"}, "slab": {"f32"}, "ws": {"x3"}, "ps": {"h2"}}[fam]


def test_every_conv_capable_tile_runs_an_exact_conv_case():
    admitting = {cfg for cfg in ALL_CFG if any(expected(p, cfg, m) for p in conv_cases(cfg if cfg in CONV_TILES else 1) for m in MODES)}
    assert admitting == set(CONV_TILES) and len(admitting) == 6 + 8 + 2 + 4
    for cfg in (c for c in CONV_TILES if family(c) in ("lds", "ws")):      # these take every geometry of the list (ws: not the upsampling)
        for p in conv_cases(cfg):
            assert any(expected(p, cfg, m) for m in MODES) or (family(cfg) == "ws" and p.conv[6]), (cfg, desc(p))


@pytest.mark.parametrize("cfg", sorted(SLAB))
def test_slab_fused_skip_connection_exact(ops, cfg):
    """K = 9 c0 + skip_c0 + skip_c1: the trailing K columns multiply the rows of skip_a0 | skip_a1 at the output pixel."""
    bn = tile(cfg)[1]
    for (h, w), n in (((3, 8), 1), ((5, 7), 3), ((1, 5), 1)):
        p = prob(N=bn, c0=32, conv=(h, w, 1, 1, 0), n=n, skip=(8, 8))
        assert expected(p, cfg, "f32")
        assert sweep(ops, p, (cfg,))
    p = prob(N=bn, c0=32, conv=(3, 8, 1, 1, 0), n=2, skip=(8, 8), splitk=2)
    if expected(p, cfg, "f32"):
        assert sweep(ops, p, (cfg,))


@pytest.mark.parametrize("cfg", PS_CONV)
def test_conv_mode_ps_split_k_exact(ops, cfg):
    """C_in = 32 with splitk = 1 and C_in = 64 with splitk = 2 (K split on 32-channel chunk boundaries)."""
    bn = tile(cfg)[1]
    for c0, sk in ((32, 1), (64, 2), (64, 1)):
        for (h, w), n in (((5, 7), 3), ((3, 8), 1), ((6, 4), 2)):
            p = prob(N=bn + 32, c0=c0, conv=(h, w, 1, 1, 0), n=n, vec=True, alpha=0.5, splitk=sk)
            assert expected(p, cfg, "h2")
            assert (cfg, "h2") in sweep(ops, p, (cfg,))
    p = prob(N=bn, c0=64, conv=(6, 4, 2, 0, 0), n=2, vec=True, splitk=2, raw=True)
    assert (cfg, "h2") in sweep(ops, p, (cfg,))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. arithmetics: aliases, the range flag
def test_lds_tile_aliases_in_the_16_bit_forms(ops):
    """dispatch_wk1: tile_cfg 3 runs as 4 and 6 as 5 (as 2 under GEGLU) in every 16-bit form -- bitwise, on random (inexact) data."""
    M, K, N = 129, 96, 132
    x, w, b = rnd(40, M, K), rnd(41, K, N) / 8.0, rnd(42, N)
    xd, wd, bd = x.cuda(), w.cuda().contiguous(), b.cuda()
    ops.pack_wsplit(wd)
    ops.pack_wsplit_h2(wd)
    wb = ops.pack_wbf16t(wd)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    # GEGLU (N % 64 == 0): tile 6 runs as tile 2, the tile of (value, gate) pairs
    Ng = 128
    wg, bg = ops.pack_geglu((rnd(43, Ng, K) / 8.0).cuda(), rnd(44, Ng).cuda())
    ops.pack_wsplit(wg)
    ops.pack_wsplit_h2(wg)
    wgb = ops.pack_wbf16t(wg)
    for mode, comp in (("bf16", 1), ("bf16i", 1), ("x3", 2), ("h2", 3)):
        outs = {}
        for cfg in (3, 4, 6, 5):
            out = torch.full((M, N), SENT, device="cuda")
            a = ops.make_igemm_args(M, N, K, xd, K, wd, out, N, M, bias=bd, tile_cfg=cfg, splitk=1, compute=comp, range_flag=flag,
                                    w_bf16t=wb if mode == "bf16i" else None)
            ops.igemm(a)
            outs[cfg] = out
        assert torch.equal(outs[3], outs[4]) and torch.equal(outs[6], outs[5]), mode
        assert not (outs[5] == SENT).any()
        gouts = {}
        for cfg in (6, 2):
            out = torch.full((M, Ng // 2), SENT, device="cuda")
            a = ops.make_igemm_args(M, Ng, K, xd, K, wg, out, Ng // 2, M, bias=bg, epi=1, tile_cfg=cfg, splitk=1, compute=comp,
                                    range_flag=flag, w_bf16t=wgb if mode == "bf16i" else None)
            ops.igemm(a)
            gouts[cfg] = out
        assert torch.equal(gouts[6], gouts[2]) and not (gouts[2] == SENT).any(), f"{mode}: GEGLU on tile 6 must be tile 2's result"
    assert int(flag) == 0


@pytest.mark.parametrize("cfg", [1, 5, 23, 27, 31, 33])
def test_f16x2_range_flag_is_raised_by_one_activation_of_1000(ops, cfg):
    bm, bn = tile(cfg)
    N = 36 if cfg in LDS else bn
    p = prob(M=33, N=N, c0=64, big=33 * 64 - 7, seed=1100)
    a, o = make(ops, p, cfg, "h2")
    if cfg in PS:                                           # the producer of the PS operand raises it (ldmk_pack_ps_h2)
        assert int(dev(ops, p).flag0) == 1
        return
    assert check(a)
    ops.igemm(a)
    guards(p, o, f"tile_cfg={cfg} h2, one activation of 1000")
    assert int(o.flag[0]) == 1, "range_flag must be raised by an activation of LDMK_F16X2_RANGE"
    q = prob(M=33, N=N, c0=64, seed=1100)
    launch_exact(ops, q, cfg, "h2")                         # the same problem without it: flag stays 0 (asserted inside)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the PS layout: padding rows, out_ps
def _poison_ps_padding(ps, M, K, planes, patterns):
    """Overwrite the rows M .. 32 ceil(M / 32) - 1 of a PS tensor (uint8 [bytes]) with 16-bit patterns, through ps_row_words."""
    words = ps.view(torch.int16)
    for i, r in enumerate(range(M, 32 * -(-M // 32))):
        idx = R.ps_row_words(r, K, planes).cuda()
        words[idx] = torch.tensor(patterns[i % len(patterns)], dtype=torch.int16, device="cuda")


@pytest.mark.parametrize("cfg,conv", [(23, False), (29, False), (31, False), (23, True)])
def test_ps_padding_rows_may_hold_anything(ops, cfg, conv):
    """ldmk.h: rows R .. 32 ceil(R / 32) - 1 of a PS tensor are padding, `any finite or non-finite content: it only reaches output rows
    that are masked`.  M = 33: rows 33..63 overwritten with NaN and Inf bit patterns (bf16: 0x7FC0, 0x7F80, 0xFF80; fp16: 0x7E00,
    0x7C00, 0xFC00) -- the output is bitwise unchanged and the guards are intact."""
    if conv:                                                # 33 stored pixels: n = 3 of 1 x 11
        p, mode = prob(N=160, c0=32, conv=(1, 11, 1, 1, 0), n=3, vec=True), "h2"
    else:
        p, mode = prob(M=33, N=160, c0=64, vec=True, rps=5), "x3"
    assert expected(p, cfg, mode)
    clean = launch_exact(ops, p, cfg, mode)
    g = dev(ops, p)
    rows = 33
    if conv:
        _poison_ps_padding(g.aps_h2[0], rows, p.c0, 2, [0x7E00, 0x7C00, -1024])
    else:
        _poison_ps_padding(g.aps[0], rows, p.K, 3, [0x7FC0, 0x7F80, -128])
    try:
        torch.cuda.synchronize()
        dirty = launch_exact(ops, p, cfg, mode)
        assert torch.equal(clean, dirty)
    finally:
        del p.g


@pytest.mark.parametrize("cfg,mode", [(c, m) for c in sorted(PS) for m in ("x3", "h2") if not (m == "h2" and c in (29, 30))])
def test_out_ps_is_pack_ps_of_the_result(ops, cfg, mode):
    """The result in the PS layout (ldc = N + 16 columns) == pack_ps of the fp32 result on every row below M; nothing behind
    ldmk_ps_bytes is written.  M = 33 (ragged block) and BM + 1."""
    bm, bn = tile(cfg)
    for M in (33, bm + 1):
        p = prob(M=M, N=bn, c0=64, vec=True, rps=5, out_ps=True)
        assert expected(p, cfg, mode)
        a, o = make(ops, p, cfg, mode)
        assert check(a)
        ops.igemm(a)
        out = guards(p, o, f"out_ps tile_cfg={cfg} {mode}")
        _exact(out[:, :M, :p.N], data(p).ref, "out next to out_ps")
        assert (o.out_ps[o.ops_bytes:] == 0x5A).all(), "out_ps was written past ldmk_ps_bytes"
        assert int(o.flag[0]) == 0
        res = torch.zeros(M, o.ldc, device="cuda")
        res[:, :p.N] = o.out[0, :M, :p.N]
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        want = ops.pack_ps(res, h2_flag=flag if mode == "h2" else None)[0]
        unpack = ops.unpack_ps_h2 if mode == "h2" else ops.unpack_ps
        for got_pl, want_pl in zip(unpack(o.out_ps[:o.ops_bytes].cpu(), M, o.ldc), unpack(want.cpu(), M, o.ldc)):
            assert torch.equal(got_pl[:, :p.N], want_pl[:, :p.N])
        unit = 2048 if mode == "h2" else 3072                                    # whole row blocks: the bytes themselves, of the
        for rb in range(M // 32):                                                # k-slabs that hold result columns only
            lo = rb * (o.ldc // 16) * unit
            assert torch.equal(o.out_ps[lo:lo + (p.N // 16) * unit], want[lo:lo + (p.N // 16) * unit])


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the paths that cannot be exact: SiLU prologue, GEGLU epilogue, both LayerNorm forms, stats_out
# (every figure is printed before it is asserted; profiles/igemm_edges_errors.txt holds the maxima of one run)
def _held(got, ref, tol, what):
    """|got - ref| <= tol + tol |ref| elementwise: torch.testing.assert_close(rtol = atol = tol), the form the existing bounds are in"""
    err = (got.double() - ref).abs()
    worst = (err / (tol + tol * ref.abs())).max().item()
    print(f"{what}: max |err| {err.max().item():.3e}, {worst:.3f} of the bound (rtol = atol = {tol:g})")
    assert worst <= 1.0, f"{what}: max |err| {err.max().item():.3e} exceeds rtol = atol = {tol:g}"


# the bounds the project holds.  F32: 1e-4 (test_ops_gpu.py: test_conv3x3, test_linear_layernorm_prologue).  BF16X3 (test_split_gpu.py):
# 5e-6 for the convolution with the SiLU prologue (test_warp_specialised_conv3x3_with_prologue_and_two_sources), 3e-6 for the linear
# forms (test_split_linear_matches_float64_like_the_fp32_form) -- taken for both LayerNorm forms and GEGLU.  F16X2: 6e-6, the
# largest absolute bound of test_f16x2_gpu.py (test_f16x2_linear_matches_float64_like_the_fp32_form), for every path.
TOL_SILU = {"f32": 1e-4, "x3": 5e-6, "h2": 6e-6}
TOL = {"f32": 1e-4, "x3": 3e-6, "h2": 6e-6}
NONEXACT_TILES = {"lds": (1, 2, 4, 5), "row": (8, 11), "slab": (14, 16), "ws": (21, 22), "ps": (23, 25, 28, 30, 33)}


def _random_rows(p, seed):
    """random operands for problem p in place of the integers (same shapes, guards and poison)"""
    d = SimpleNamespace()
    shp = (p.n, p.conv[0], p.conv[1]) if p.conv else (p.M,)
    d.x0 = rnd(seed, 1, *shp, p.c0) + 0.3
    d.x1 = None
    d.w = rnd(seed + 1, 1, p.K, p.N) / p.K ** 0.5
    d.bias = 0.1 * rnd(seed + 2, p.N)
    d.vec, d.res, d.skip0, d.skip1 = None, None, None, None
    d.coef = torch.stack([1.0 + 0.2 * rnd(seed + 3, p.n, p.c0), 0.3 * rnd(seed + 4, p.n, p.c0)], 1).contiguous() if p.tf in (TF_AFFINE, TF_SILU) else None
    return d


@pytest.mark.parametrize("cfg", [1, 2, 4, 5, 21, 22])
def test_silu_prologue_at_the_edges(ops, cfg):
    """GroupNorm scale / shift + SiLU while staging (conv mode 5x7, n = 3: M = 105 with sample boundaries inside the tile, and rows
    mode M = 33 / BM + 1, K = 32) against float64."""
    bm, bn = tile(cfg)
    N = 36 if cfg in LDS else bn
    cases = [prob(N=N, c0=32, conv=(5, 7, 1, 1, 0), n=3, tf=TF_SILU, res=False)] + \
            [prob(M=m, N=N, c0=32, tf=TF_SILU, res=False, rps=5) for m in (33, bm + 1)]
    for i, p in enumerate(cases):
        d = p.d = _random_rows(p, 50 + i)
        xa = F.silu(R.concat_affine(d.x0[0], None, d.coef)) if p.conv else None
        if p.conv:
            A = R.conv_operand(xa, *p.conv[4:])[0]
        else:
            smp = torch.arange(p.M) // p.rps
            A = F.silu(d.x0[0].double() * d.coef[smp, 0].double() + d.coef[smp, 1].double())
        d.A = [A]
        d.ref = R.igemm_ref(A, d.w[0], 1.0, d.bias)[None]
        for mode in (("f32", "x3", "h2") if cfg in LDS else ("x3",)):
            assert expected(p, cfg, mode)
            a, o = make(ops, p, cfg, mode)
            assert check(a)
            ops.igemm(a)
            out = guards(p, o, f"SiLU prologue tile_cfg={cfg} {mode}")
            _held(out[0, :p.M, :p.N], d.ref[0], TOL_SILU[mode], f"SiLU prologue tile_cfg={cfg} {mode} M={p.M}")


def _ln_problem(ops, M, K, N, geglu, seed):
    x = rnd(seed, M, K) + 0.5 * rnd(seed + 1, M, 1)
    w, b = rnd(seed + 2, N, K) / K ** 0.5, 0.1 * rnd(seed + 3, N)
    gamma, beta = 1.0 + 0.2 * rnd(seed + 4, K), 0.2 * rnd(seed + 5, K)
    wp, bp = ops.pack_geglu(w.cuda(), b.cuda()) if geglu else (ops.pack_linear(w.cuda()), b.cuda())
    y = F.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-5) @ wp.cpu().double() + bp.cpu().double()   # packed column order
    ref = R.geglu_ref(y, N // 2) if geglu else y
    return x, wp, bp, gamma, beta, ref


@pytest.mark.parametrize("fam", sorted(NONEXACT_TILES))
def test_layernorm_forms_and_geglu_at_the_edges(ops, fam):
    """M = 33 and BM + 1, K = 32, guarded outputs, float64 reference: the folded LayerNorm (every family) with and without the GEGLU
    epilogue, and the staging LayerNorm prologue (LDS / row / ws tiles).  What must run is written down per tile (below) and held against
    the support table and ldmk_igemm_check: a table or a check that refused a LayerNorm form fails the test, it cannot thin it out."""
    modes = {"lds": ("f32", "x3", "h2"), "row": ("f32",), "slab": ("f32",), "ws": ("x3",), "ps": ("x3", "h2")}[fam]
    want, ran = set(), set()
    for cfg in NONEXACT_TILES[fam]:
        # GEGLU needs (value, gate) tile pairs: every LDS tile (3..6 are redirected), an even TN elsewhere, tile 22 of the ws pair
        geglu_ok = {"lds": True, "row": cfg in ROW and ROW[cfg][1] % 2 == 0, "slab": cfg in SLAB and SLAB[cfg][1] % 2 == 0,
                    "ws": cfg == 22, "ps": cfg in PS_EVEN_TN}[fam]
        for mode in modes:
            if mode == "h2" and cfg in (29, 30):             # the warp-specialised pre-split tiles exist in bf16x3 only
                continue
            want.add((cfg, mode, TF_LNF, False))
            if fam in ("lds", "row", "ws"):                  # the staging prologue is not built for the slab and pre-split tiles
                want.add((cfg, mode, TF_LN, False))
            if geglu_ok:
                want.add((cfg, mode, TF_LNF, True))
    for cfg in NONEXACT_TILES[fam]:
        bm, bn = tile(cfg)
        for M in (33, bm + 1):
            for geglu in (False, True):
                N, K = (2 * bn if geglu and bn % 64 else bn), 32
                if fam == "lds":
                    N = 128 if geglu else 36
                x, wp, bp, gamma, beta, ref = _ln_problem(ops, M, K, N, geglu, 70)
                xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
                st = ops.ln_stats(xd)
                w2, cs, b2 = ops.fold_layernorm(wp, gd, bd, bp)
                nc = N // 2 if geglu else N
                for mode in modes:
                    for form in (TF_LNF, TF_LN):
                        p = prob(M=M, N=N, c0=K, tf=form, geglu=geglu, res=False)
                        if form == TF_LN and geglu:          # (the transformer block folds the LayerNorm in front of GEGLU: one form)
                            continue
                        runs = (cfg, mode, form, geglu) in want
                        assert expected(p, cfg, mode) == runs, (cfg, mode, form, geglu)
                        if not runs:
                            continue
                        out = torch.full((M + 32, nc + 12), SENT, device="cuda")
                        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
                        w_, b_ = (w2, b2) if form == TF_LNF else (wp, bp)
                        kw = dict(tf=form, row_stats=st, bias=b_, epi=1 if geglu else 0, tile_cfg=cfg, splitk=1)
                        kw.update(dict(ln_colsum=cs) if form == TF_LNF else dict(ln_gamma=gd, ln_beta=bd))
                        if fam in ("row", "slab"):
                            kw.update(w_frag=ops.pack_wfrag(w_))
                        if fam == "ps":
                            aps = ops.pack_ps(xd, h2_flag=flag if mode == "h2" else None)
                            a = ops.make_igemm_args(M, N, K, None, K, w_, out, nc + 12, M, a_ps=aps, w_ps=ops.pack_wps(w_, h2=mode == "h2"),
                                                    range_flag=flag, **kw)
                        else:
                            if mode == "x3":
                                ops.pack_wsplit(w_)
                            if mode == "h2":
                                ops.pack_wsplit_h2(w_)
                            a = ops.make_igemm_args(M, N, K, xd, K, w_, out, nc + 12, M, compute=MODES[mode], range_flag=flag, **kw)
                        assert check(a), (cfg, mode, form, geglu)
                        ops.igemm(a)
                        oc = out.cpu()
                        assert (oc[M:] == SENT).all() and (oc[:, nc:] == SENT).all(), "LayerNorm / GEGLU launch wrote outside its result"
                        assert int(flag) == 0
                        ran.add((cfg, mode, form, geglu))
                        _held(oc[:M, :nc], ref, TOL[mode], f"{'folded' if form == TF_LNF else 'staged'} LayerNorm{' + GEGLU' if geglu else ''} "
                                                     f"tile_cfg={cfg} {mode} M={M}")
    assert ran == want, (sorted(want - ran), sorted(ran - want))


@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5, 6, 15, 16, 21, 22, 23, 27, 29, 31])
def test_stats_out_records_at_the_edges(ops, cfg):
    """M = 32 and 96, rows_per_sample = 32, splitk in {1, 2}: the sums sum(y) and sum(y^2) per 32-row tile and column, rebuilt in
    float64 from the three stored floats (shift, sum(y - shift), sum((y - shift)^2)), against float64 sums of the reference output at the
    relative 1e-5 test_igemm_emits_groupnorm_partials holds on the coefficients; nothing behind the M / 32 tiles is written."""
    bm, bn = tile(cfg)
    fam = family(cfg)
    N = 36 if fam == "lds" else bn
    mode = {"lds": "f32", "slab": "f32", "ws": "x3", "ps": "x3"}[fam]
    for M in (32, 96):
        for sk in (1, 2):
            p = prob(M=M, N=N, c0=64, rps=32, vec=True, stats=True, splitk=sk, seed=1200)
            assert expected(p, cfg, mode)
            d = data(p)
            a, o = make(ops, p, cfg, mode)
            assert check(a)
            ops.igemm(a)
            out = guards(p, o, f"stats_out tile_cfg={cfg} splitk={sk}")
            _exact(out[:, :M, :N], d.ref, "output next to stats_out")
            q = o.stats[:o.nrec].cpu().double().view(M // 32, N, 3)
            s1 = q[..., 1] + 32 * q[..., 0]
            s2 = q[..., 2] + 2 * q[..., 0] * q[..., 1] + 32 * q[..., 0] ** 2
            y = d.ref[0].view(M // 32, 32, N)
            r1, r2 = y.sum(1), (y * y).sum(1)
            e1 = ((s1 - r1).abs() / r1.abs().clamp_min(1.0)).max().item()          # (integer outputs: |sum| >= 1 unless it is exactly 0)
            e2 = ((s2 - r2).abs() / r2.clamp_min(1.0)).max().item()
            print(f"stats_out tile_cfg={cfg} M={M} splitk={sk}: sum {e1:.2e}, sum of squares {e2:.2e} (relative, bound 1e-5)")
            assert e1 <= 1e-5 and e2 <= 1e-5
