"""Edge shapes and exact arithmetic of the training-step kernels (csrc/wgrad.hip, attention_train.hip, backward.hip and the
bf16 backward entry points of attention_bf16.hip), below whole-UNet level.

Two kinds of check.  (1) Integer operands in [-2, 2]: every product and partial sum is an integer far below 2^24 (and, for
the bf16 matrix cores, every operand is bf16-exact), so the weight gradient, its slab reduce, the fused bias sums, the
data gradient and the column sums must equal the float64 reference BITWISE -- one wrong row, column, tap or slab shows.
(2) float64 autograd of the same op at token counts / widths on the tile edges, with the bounds of test_backward_gpu.py
and test_bf16_gpu.py (stated per test)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rnd
from test_ops_gpu import nhwc, ops  # noqa: F401  (the `ops` fixture)

pytestmark = pytest.mark.gpu

SENT = -7.0          # sentinel for memory a kernel must not write (an integer, so it also serves the exact tests)


@pytest.fixture(autouse=True)
def _autograd_on():
    """The reference side of these tests is autograd; other test modules switch it off process-wide."""
    with torch.enable_grad():
        yield


def _ints(seed, *shape, lo=-2, hi=2):
    return torch.from_numpy(np.random.RandomState(seed).randint(lo, hi + 1, size=shape).astype(np.float32))


def _close(got, ref, rtol, what):
    ref = ref.detach().to(torch.float64)
    err = (got.detach().cpu().to(torch.float64) - ref).abs().max().item()
    bound = rtol * max(ref.abs().max().item(), 1e-30)
    print(f"{what}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def _exact(got, ref64, what):
    ref = ref64.to(torch.float32)
    assert ref.double().equal(ref64.double()), f"{what}: reference is not fp32-exact (test bug)"
    got = got.detach().cpu()
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {ref.numel()} elements differ, first at {bad[0].tolist()}: "
                             f"{got[tuple(bad[0])].item()} vs {ref[tuple(bad[0])].item()}")


def _compute(mode):
    from dsml_thesis_amd import train_ops as T
    return T.set_compute(mode)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. weight gradient, exact
def _wgrad_tile(Kw, N):
    """Mirror of wgrad_cfg (csrc/wgrad.hip): the tile the library picks for a [Kw][N] weight gradient."""
    waste = lambda v, b: np.float32(-(-v // b) * b) / np.float32(v)
    w = [waste(Kw, 128) * waste(N, 160), waste(Kw, 160) * waste(N, 128), waste(Kw, 128) * waste(N, 128) * np.float32(1.08),
         waste(Kw, 128) * waste(N, 32) * np.float32(1.5)]
    return ["128x160", "160x128", "128x128", "128x32"][int(np.argmin(w))]      # argmin: first minimum, like the `<` chain


def _launch_wgrad(T, R, Kw, N, a, dy, dw, splitr=0, dbias=None, batch=1, **kw):
    """ldmk_wgrad with its own workspace of exactly the size the split needs; returns the split used."""
    w = T.wgrad_args(R, Kw, N, a, dy, dw, splitr=splitr, dbias=dbias, batch=batch, **kw)
    sr = T.wgrad_workspace_elems(w)[0] if splitr == 0 else splitr
    need = sr * max(1, batch) * (Kw + (1 if dbias is not None else 0)) * N if sr > 1 else 0
    ws = torch.empty(max(need, 1), device="cuda")
    w.splitr, w.ws, w.ws_elems = sr, ws.data_ptr(), need
    T.wgrad(w)
    return sr


# (R, Kw, N) -> (tile of wgrad_cfg, planner's split)
WGRAD_ROWS = {(97, 128, 128): ("128x128", 1), (2049, 1152, 128): ("128x128", 8), (33, 164, 132): ("128x160", 1),
              (257, 288, 128): ("160x128", 1), (300, 288, 32): ("128x32", 1), (31, 4, 4): ("128x32", 1), (1, 8, 4): ("128x32", 1)}


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("R,Kw,N", list(WGRAD_ROWS))
def test_wgrad_rows_exact(ops, R, Kw, N, compute):
    """dW = A^T dY and dbias = column sums of dY on integer operands: bitwise the float64 result for every tile of wgrad_cfg,
    tails in R, Kw and N, every split (planner's, none, 2, 3, 9 and 17 slabs -- the second trip of the reduce's 8-at-a-time loop
    -- and one slab more than there are 32-row slices, i.e. an empty slab), accumulate, alpha and leading dimensions."""
    from dsml_thesis_amd import train_ops as T
    tile, plan = WGRAD_ROWS[(R, Kw, N)]
    assert _wgrad_tile(Kw, N) == tile
    a, dy = _ints(500, R, Kw), _ints(501, R, N)
    ref, ref_b = a.double().t() @ dy.double(), dy.double().sum(0)
    ad, dyd = a.cuda(), dy.cuda()
    iters = (R + 31) // 32
    splits = [0, 1] + [s for s in (2, 3, 9, 17, iters + 1) if s <= 256]
    _compute(compute)
    try:
        sr, _ = T.wgrad_workspace_elems(T.wgrad_args(R, Kw, N, ad, dyd, torch.empty(Kw, N, device="cuda")))
        assert sr == plan, f"wgrad planner: split {sr}, the case was chosen for {plan}"
        first = None
        for s in splits:
            for with_bias in (False, True):
                dw = torch.full((Kw, N), SENT, device="cuda")
                db = torch.full((N,), SENT, device="cuda") if with_bias else None
                _launch_wgrad(T, R, Kw, N, ad, dyd, dw, splitr=s, dbias=db)
                _exact(dw, ref, f"wgrad rows splitr={s} bias={with_bias}")
                if with_bias:
                    _exact(db, ref_b, f"fused bias gradient splitr={s}")
            first = dw if first is None else first
            assert torch.equal(first, dw), "wgrad must be bitwise reproducible across calls and splits of exact data"
        # a split combined with accumulate, alpha != 1 and leading dimensions (padding columns of dW keep their sentinel)
        prior, prior_b = _ints(502, Kw, N, lo=-5, hi=5), _ints(503, N, lo=-5, hi=5)
        abuf, dybuf = torch.full((R, Kw + 8), 3.0), torch.full((R, N + 4), 3.0)      # padding a kernel must not read as data
        abuf[:, :Kw], dybuf[:, :N] = a, dy
        abuf, dybuf = abuf.cuda(), dybuf.cuda()
        for s in (1, 3, 9):
            for alpha in (1.0, 0.5, 2.0):
                dw, db = prior.cuda(), prior_b.cuda()
                _launch_wgrad(T, R, Kw, N, ad, dyd, dw, splitr=s, dbias=db, accumulate=True, alpha=alpha)
                _exact(dw, prior.double() + alpha * ref, f"wgrad accumulate splitr={s} alpha={alpha}")
                _exact(db, prior_b.double() + alpha * ref_b, f"bias accumulate splitr={s} alpha={alpha}")
            dwbuf = torch.full((Kw, N + 12), SENT, device="cuda")
            db = torch.full((N,), SENT, device="cuda")
            _launch_wgrad(T, R, Kw, N, abuf, dybuf, dwbuf, splitr=s, dbias=db, alpha=0.5, lda=Kw + 8, ldy=N + 4, ldw=N + 12)
            _exact(dwbuf[:, :N], 0.5 * ref, f"wgrad lda/ldy/ldw splitr={s}")
            _exact(db, 0.5 * ref_b, f"bias lda/ldy/ldw splitr={s}")
            assert (dwbuf[:, N:] == SENT).all(), f"splitr={s}: the padding columns of dW were written"
            dwbuf[:, :N] = prior.cuda()
            _launch_wgrad(T, R, Kw, N, abuf, dybuf, dwbuf, splitr=s, accumulate=True, lda=Kw + 8, ldy=N + 4, ldw=N + 12)
            _exact(dwbuf[:, :N], prior.double() + ref, f"wgrad accumulate + ldw splitr={s}")
            assert (dwbuf[:, N:] == SENT).all(), f"splitr={s}: the padding columns of dW were written (accumulate)"
    finally:
        _compute("f32")


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_wgrad_batched_split_exact(ops, compute):
    """Z = 3 problems over blockIdx.z with a row split: slab (bz * splitr + ks) addressing, and a dw_bstride wider than one
    problem's Kw * ldw whose gap keeps its sentinel."""
    from dsml_thesis_amd import train_ops as T
    Z, R, Kw, N = 3, 96, 64, 32
    a, dy = _ints(510, Z, R, Kw), _ints(511, Z, R, N)
    ref = a.double().transpose(1, 2) @ dy.double()
    prior = _ints(512, Z, Kw, N, lo=-5, hi=5)
    ad, dyd = a.cuda(), dy.cuda()
    bstride = Kw * N + 40
    _compute(compute)
    try:
        for s in (1, 3):
            for acc in (False, True):
                out = torch.full((Z, bstride), SENT, device="cuda")
                if acc:
                    out[:, :Kw * N] = prior.view(Z, -1).cuda()
                _launch_wgrad(T, R, Kw, N, ad, dyd, out, splitr=s, batch=Z, a_bstride=R * Kw, dy_bstride=R * N, dw_bstride=bstride,
                              accumulate=acc, alpha=2.0 if acc else 1.0)
                want = prior.double() + 2.0 * ref if acc else ref
                _exact(out[:, :Kw * N].reshape(Z, Kw, N), want, f"batched wgrad splitr={s} accumulate={acc}")
                assert (out[:, Kw * N:] == SENT).all(), f"batched wgrad splitr={s}: the gap between problems was written"
    finally:
        _compute("f32")


# (n, cin, cout, h, w, stride, upsample, pad_lo)
CONV_CASES = [(2, 32, 36, 3, 8, 1, False, 1),        # power-of-two out_w, out_h*out_w = 24 is not
              (1, 64, 32, 4, 6, 1, False, 1),        # non-power-of-two out_w
              (2, 32, 32, 5, 7, 2, False, 1),
              (1, 32, 64, 6, 4, 2, False, 0),        # asymmetric pad (the Downsample convolution): pad (0, 1, 0, 1), padding 0
              (1, 32, 32, 3, 5, 1, True, 1),
              (1, 128, 128, 4, 4, 1, False, 1)]      # Kw = 1152, N = 128: the 128x128 tile


@functools.lru_cache(maxsize=None)
def _conv_ref(case):
    """Integer x, w, dy of a 3x3 convolution and its float64 autograd gradients (computed once per geometry)."""
    n, cin, cout, h, w, stride, ups, pad_lo = case
    x = _ints(520, n, cin, h, w).double().requires_grad_(True)
    wt = _ints(521, cout, cin, 3, 3).double().requires_grad_(True)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if ups else x
    if pad_lo == 0:
        y = F.conv2d(F.pad(xin, (0, 1, 0, 1)), wt, None, stride=stride, padding=0)
    else:
        y = F.conv2d(xin, wt, None, stride=stride, padding=1)
    dy = _ints(522, *y.shape)
    y.backward(dy.double())
    return x.detach().float(), wt.detach().float(), dy, wt.grad, x.grad


def _pack_ref(w):
    """OIHW -> [I/32][9][32][O] rows, what ops.pack_conv3x3 documents."""
    o, i = w.shape[:2]
    return w.reshape(o, i // 32, 32, 9).permute(1, 3, 2, 0).reshape(9 * i, o)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("case", CONV_CASES)
def test_wgrad_conv_exact(ops, case, compute):
    """Conv-mode weight gradient in the packed forward layout, non-square maps: the rps_shift / ow_shift fast paths in every
    combination, stride 2, asymmetric pad, nearest-x2 upsampling; with the fused bias gradient, plain and accumulating."""
    from dsml_thesis_amd import train_ops as T
    n, cin, cout, h, w, stride, ups, pad_lo = case
    x, _, dy, wgrad, _ = _conv_ref(case)
    if cin == 128:
        assert _wgrad_tile(9 * cin, cout) == "128x128"
    ref = _pack_ref(wgrad)
    assert torch.equal(ops.pack_conv3x3(wgrad.float().cuda()).cpu(), ref.float())
    ref_b = dy.double().sum((0, 2, 3))
    xd, dyd = nhwc(x), nhwc(dy)
    prior, prior_b = _ints(523, 9 * cin, cout, lo=-5, hi=5), _ints(524, cout, lo=-5, hi=5)
    _compute(compute)
    try:
        dw, db = torch.full((9 * cin, cout), SENT, device="cuda"), torch.full((cout,), SENT, device="cuda")
        T.wgrad_conv3x3(xd, dyd, stride=stride, pad_lo=pad_lo, upsample=ups, dw=dw, dbias=db)
        _exact(dw, ref, "conv wgrad")
        _exact(db, ref_b, "conv bias gradient")
        dw2, db2 = prior.cuda(), prior_b.cuda()
        T.wgrad_conv3x3(xd, dyd, stride=stride, pad_lo=pad_lo, upsample=ups, dw=dw2, dbias=db2, accumulate=True)
        _exact(dw2, prior.double() + ref, "conv wgrad accumulate")
        _exact(db2, prior_b.double() + ref_b, "conv bias gradient accumulate")
        # explicit splits, one of them with more slabs than 32-row slices
        oh, ow = dy.shape[2:]
        for s in (2, 9):
            dw3 = torch.full((9 * cin, cout), SENT, device="cuda")
            _launch_wgrad(T, n * oh * ow, 9 * cin, cout, xd, dyd, dw3, splitr=s, c=cin,
                          conv=(h, w, oh, ow, stride, pad_lo, 1 if ups else 0))
            _exact(dw3, ref, f"conv wgrad splitr={s}")
    finally:
        _compute("f32")


# conv3x3_dgrad supports pad 1 and channel counts that are multiples of 32: CONV_CASES without cout = 36 and pad_lo = 0, plus the
# power-of-two-width geometry of the first case with 32 output channels
DGRAD_CASES = [(2, 32, 32, 3, 8, 1, False, 1)] + [c for c in CONV_CASES if c[2] % 32 == 0 and c[7] == 1]


@pytest.mark.parametrize("case,compute", [(c, "f32") for c in DGRAD_CASES] + [(DGRAD_CASES[1], "bf16"), (DGRAD_CASES[2], "bf16")])
def test_conv3x3_dgrad_exact(ops, case, compute):
    """Data gradient through the mirrored-tap weights (pack_dgrad3x3), non-square; plain, and accumulated onto a non-zero
    tensor through residual=out as the trainer does.  Integer weights and dy: exact in fp32 and in bf16 compute."""
    from dsml_thesis_amd import train_ops as T
    n, cin, cout, h, w, stride, ups, _ = case
    _, wt, dy, _, xgrad = _conv_ref(case)
    dyd = nhwc(dy)
    wd = T.pack_dgrad3x3(ops.pack_conv3x3(wt.cuda()), cin, cout)
    assert torch.equal(wd.cpu(), _pack_ref(wt.flip(2, 3).transpose(0, 1).contiguous())), "pack_dgrad3x3: mirrored taps, swapped channels"
    hh, ww = (2 * h, 2 * w) if ups else (h, w)
    ref = xgrad.permute(0, 2, 3, 1)
    prior = _ints(525, n, hh, ww, cin, lo=-5, hi=5)
    _compute(compute)
    try:
        dx = T.conv3x3_dgrad(dyd, wd, (hh, ww), stride=stride)
        out = prior.cuda()
        T.conv3x3_dgrad(dyd, wd, (hh, ww), stride=stride, out=out, residual=out)
    finally:
        _compute("f32")
    if ups:
        _exact(T.sumpool2(dx), ref, "conv dgrad (sumpool2 of the upsampled gradient)")
        _exact(T.sumpool2(out), ref + prior.double().view(n, h, 2, w, 2, cin).sum((2, 4)), "conv dgrad accumulate (upsampled)")
        acc = prior[:, :h, :w].contiguous().cuda()
        T.sumpool2(dx, out=acc, accumulate=True)
        _exact(acc, ref + prior[:, :h, :w].double(), "sumpool2 accumulate")
    else:
        _exact(dx, ref, "conv dgrad")
        _exact(out, ref + prior.double(), "conv dgrad accumulate (residual=out)")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. flash attention backward at the tile edges
@functools.lru_cache(maxsize=None)
def _attn_ref(n, tokens, heads, qk_scale=1.0):
    """(qkv fp32, dout fp32, out, lse, d(qkv)) -- the last three float64 autograd of softmax(Q K^T / sqrt(32)) V."""
    C = heads * 32
    qkv32 = rnd(530, n * tokens, 3 * C)
    qkv32[:, :2 * C] *= qk_scale
    qkv = qkv32.double().requires_grad_(True)
    dout = rnd(531, n * tokens, C)
    q, k, v = qkv.view(n, tokens, 3, heads, 32).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) * 32 ** -0.5
    att = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(n * tokens, C)
    att.backward(dout.double())
    return qkv32, dout, att.detach(), torch.logsumexp(s, -1).detach(), qkv.grad


def _attn_run(n, tokens, heads, qkv, dout, compute):
    from dsml_thesis_amd import train_ops as T
    qd, dd = qkv.cuda(), dout.cuda()
    _compute(compute)
    try:
        out, lse = T.attn_self_lse(qd, n, tokens, heads)
        dqkv = T.attn_self_bwd(qd, out, dd, lse, n, tokens, heads)
        again = T.attn_self_bwd(qd, out, dd, lse, n, tokens, heads)
    finally:
        _compute("f32")
    assert torch.equal(dqkv, again), "attention backward must be bitwise reproducible"
    return out, lse, dqkv


def _rel_l2(got, ref):
    return ((got.detach().double().cpu() - ref).norm() / ref.norm()).item()


# token counts on the edges of the 32-key sub-tile, the 64-row staged tile and the 128-row workgroup
ATTN_EDGES = [(1, t, 2) for t in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129)] + [(2, 65, 3)]


@pytest.mark.parametrize("n,tokens,heads", ATTN_EDGES)
def test_attention_backward_edges_fp32(n, tokens, heads):
    """Bounds of test_attention_backward: 2e-5 out, 1e-5 lse, 3e-5 d(qkv), relative to max |ref|."""
    qkv, dout, att, lse_ref, grad = _attn_ref(n, tokens, heads)
    out, lse, dqkv = _attn_run(n, tokens, heads, qkv, dout, "f32")
    _close(out, att, 2e-5, "attention forward (lse variant)")
    _close(lse, lse_ref, 1e-5, "log-sum-exp")
    _close(dqkv, grad, 3e-5, "flash attention backward")


def test_attention_backward_fp32_rows_do_not_depend_on_the_batch():
    """A ragged count (65): appending a second sample must not change a bit of the first sample's rows."""
    qkv, dout, *_ = _attn_ref(2, 65, 3)
    out2, lse2, d2 = _attn_run(2, 65, 3, qkv, dout, "f32")
    out1, lse1, d1 = _attn_run(1, 65, 3, qkv[:65].contiguous(), dout[:65].contiguous(), "f32")
    assert torch.equal(out1, out2[:65]) and torch.equal(lse1[0], lse2[0]) and torch.equal(d1, d2[:65])


@pytest.mark.parametrize("n,tokens,heads", ATTN_EDGES)
def test_attention_backward_edges_bf16(n, tokens, heads):
    """Bounds of test_bf16_attention_forward_and_backward: relative L2 1.5e-2 (out, d(qkv)), 2e-2 per part, lse 2e-2 absolute.
    tokens = 1: softmax over one key is the constant 1, so dq and dk are exactly zero in the reference; their relative error
    is undefined (reference norm below 1e-12), the kernel's values must be below 1e-6 absolute and only dv is compared.  No
    other case may skip a relative check.

    The single-token case is what holds D = rowsum(dO o O) to the rounding of dP = dO V^T: with the unrounded dO in D, dS was the
    rounding difference (dO - bf16(dO)) . V instead of zero (max |dq| 4.8e-3, max |dk| 5.9e-3 before attn_bf16_rowdot_kernel)."""
    qkv, dout, att, lse_ref, grad = _attn_ref(n, tokens, heads)
    out, lse, dqkv = _attn_run(n, tokens, heads, qkv, dout, "bf16")
    e_out, e_lse = _rel_l2(out, att), (lse.double().cpu() - lse_ref).abs().max().item()
    print(f"bf16 attention n={n} tokens={tokens} heads={heads}: out {e_out:.2e}, lse {e_lse:.2e}")
    assert e_out < 1.5e-2 and e_lse < 2e-2
    errs = {}
    for name, part, ref in zip("qkv", dqkv.double().cpu().chunk(3, dim=1), grad.chunk(3, dim=1)):
        if ref.norm().item() < 1e-12:
            assert tokens == 1 and name in "qk", "only the single-token gradient of q and k is exactly zero"
            errs[name] = part.abs().max().item()
            print(f"  d{name}: reference is zero, max |value| {errs[name]:.2e}")
            continue
        errs[name] = ((part - ref).norm() / ref.norm()).item()
        print(f"  d{name}: relative L2 {errs[name]:.2e}")
    for name, e in errs.items():
        assert e < (1e-6 if tokens == 1 and name in "qk" else 2e-2), (name, e)
    if tokens > 1:
        assert _rel_l2(dqkv, grad) < 1.5e-2


# Peaked rows: q and k scaled by 3 -> logits with a standard deviation near 9, most rows close to one-hot; exp(s - lse) spans the
# fp32 range.  The bounds come from the arithmetic, not from the kernels.  fp32: the flash formula (P = exp(S - lse), dV = P^T dO,
# dP = dO V^T, D = rowsum(dO o O), dS = P o (dP - D), dQ = scale dS K, dK = scale dS^T Q) evaluated in plain fp32 torch on the CPU
# against float64, relative to max |ref|; 4x that (summation order, __expf), floored at the unit-scale bound.  bf16: the same
# formula in float64 with every matrix-core operand (Q, K, V, dO, P, dS) rounded to bf16, against the unrounded float64,
# relative L2; 2x that.
PEAK = (1, 129, 2, 3.0)
# fp32, measured with the fp32 torch formula: out 1.64e-6, lse 2.14e-7, d(qkv) 2.18e-6; 4x is below the unit-scale bounds, which hold
PEAK_F32 = {"out": 2e-5, "lse": 1e-5, "dqkv": 3e-5}
# bf16, measured with the rounded-operand float64 model: out 7.24e-3, d(qkv) 1.484e-2, worst part (dq) 1.765e-2, lse 5.86e-2
# absolute (a logit of magnitude ~30 carries ~2^-9 of relative operand rounding); 2x, out floored at the unit-scale 1.5e-2
PEAK_BF16 = {"out": 1.5e-2, "dqkv": 2.97e-2, "part": 3.53e-2, "lse": 1.17e-1}


def test_attention_backward_peaked_rows_fp32():
    n, tokens, heads, sc = PEAK
    qkv, dout, att, lse_ref, grad = _attn_ref(n, tokens, heads, sc)
    out, lse, dqkv = _attn_run(n, tokens, heads, qkv, dout, "f32")
    assert torch.isfinite(out).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all()
    _close(out, att, PEAK_F32["out"], "peaked attention forward")
    _close(lse, lse_ref, PEAK_F32["lse"], "peaked log-sum-exp")
    _close(dqkv, grad, PEAK_F32["dqkv"], "peaked flash attention backward")


def test_attention_backward_peaked_rows_bf16():
    """Peaked rows are what holds the dK / dV kernel to the forward's roundings of the scores, bf16(scale q) . bf16(k): with
    bf16(q) . bf16(scale k) every P = exp(s - lse) of dK and dV was off by ~2^-9 |s| (dk, dv 3.8e-2 against a model value of 1.7e-2 / 6.9e-3)."""
    n, tokens, heads, sc = PEAK
    qkv, dout, att, lse_ref, grad = _attn_ref(n, tokens, heads, sc)
    out, lse, dqkv = _attn_run(n, tokens, heads, qkv, dout, "bf16")
    assert torch.isfinite(out).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all()
    e_out, e_lse, e_grad = _rel_l2(out, att), (lse.double().cpu() - lse_ref).abs().max().item(), _rel_l2(dqkv, grad)
    parts = [_rel_l2(p, r) for p, r in zip(dqkv.chunk(3, dim=1), grad.chunk(3, dim=1))]
    print(f"peaked bf16 attention: out {e_out:.2e}, lse {e_lse:.2e}, dqkv {e_grad:.2e}, parts {parts}")
    assert e_out < PEAK_BF16["out"] and e_lse < PEAK_BF16["lse"] and e_grad < PEAK_BF16["dqkv"]
    assert max(parts) < PEAK_BF16["part"]


# ---------------------------------------------------------------------------------------------------------------------------
# 3. cross-attention backward with leading dimensions
@pytest.mark.parametrize("L_ctx", [1, 3, 77])
def test_cross_attention_backward_strided(L_ctx):
    """q, k, v, dout and the gradients as column slices of wider buffers: the gradients carry the row stride of their inputs,
    the unused columns of their parents keep a sentinel, and the values are bitwise those of contiguous inputs."""
    from dsml_thesis_amd import train_ops as T
    from dsml_thesis_amd.lib import LdmkError
    n, tokens, heads = 2, 37, 2
    C_ = heads * 32
    q = rnd(540, n * tokens, C_).double().requires_grad_(True)
    k = rnd(541, n * L_ctx, C_).double().requires_grad_(True)
    v = rnd(542, n * L_ctx, C_).double().requires_grad_(True)
    qh = q.view(n, tokens, heads, 32).permute(0, 2, 1, 3)
    kh = k.view(n, L_ctx, heads, 32).permute(0, 2, 1, 3)
    vh = v.view(n, L_ctx, heads, 32).permute(0, 2, 1, 3)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * 32 ** -0.5, -1)
    out = (p @ vh).permute(0, 2, 1, 3).reshape(n * tokens, C_)
    dout = rnd(543, n * tokens, C_)
    out.backward(dout.double())
    qbuf, kvbuf, dobuf = (torch.full(s, 3.0, device="cuda") for s in ((n * tokens, 96), (n * L_ctx, 192), (n * tokens, 96)))
    qs, ks, vs, dos = qbuf[:, :C_], kvbuf[:, :C_], kvbuf[:, C_:2 * C_], dobuf[:, 16:16 + C_]
    qs.copy_(q.detach().float()); ks.copy_(k.detach().float()); vs.copy_(v.detach().float()); dos.copy_(dout)
    # gradients into slices of sentinel-filled parents
    dqbuf, dkvbuf = torch.full((n * tokens, 96), SENT, device="cuda"), torch.full((n * L_ctx, 192), SENT, device="cuda")
    dq, dk, dv = T.attn_cross_bwd(qs, ks, vs, dos, n, tokens, L_ctx, heads, dq=dqbuf[:, :C_], dk=dkvbuf[:, :C_], dv=dkvbuf[:, C_:2 * C_])
    _close(dq, q.grad, 3e-5, "strided cross attention dq")
    _close(dk, k.grad, 3e-5, "strided cross attention dk")
    _close(dv, v.grad, 3e-5, "strided cross attention dv")
    assert (dqbuf[:, C_:] == SENT).all() and (dkvbuf[:, 2 * C_:] == SENT).all(), "columns outside the gradient slices were written"
    # gradients allocated by the wrapper: the row stride of their inputs, a guard allocated right after them stays intact
    dq2, dk2, dv2 = T.attn_cross_bwd(qs, ks, vs, dos, n, tokens, L_ctx, heads)
    assert dq2.stride() == qs.stride() and dk2.stride() == ks.stride() and dv2.stride() == vs.stride()
    for t_ in (dq2, dk2, dv2):
        assert t_.untyped_storage().nbytes() >= 4 * ((t_.shape[0] - 1) * t_.stride(0) + C_)
    assert torch.equal(dq2, dq) and torch.equal(dk2, dk) and torch.equal(dv2, dv)
    # contiguous inputs: bitwise the same values
    dq3, dk3, dv3 = T.attn_cross_bwd(qs.contiguous(), ks.contiguous(), vs.contiguous(), dos.contiguous(), n, tokens, L_ctx, heads)
    assert dq3.is_contiguous() and torch.equal(dq3, dq) and torch.equal(dk3, dk) and torch.equal(dv3, dv)
    # one leading dimension for k and v
    with pytest.raises(LdmkError, match="row stride"):
        T.attn_cross_bwd(qs, ks, vs.contiguous(), dos, n, tokens, L_ctx, heads, dq=dqbuf[:, :C_], dk=dkvbuf[:, :C_])
    with pytest.raises(LdmkError, match="strides"):
        T.attn_cross_bwd(qs, ks, vs, dos, n, tokens, L_ctx, heads, dq=torch.empty(n * tokens, C_, device="cuda"))
    assert (dqbuf[:, C_:] == SENT).all() and torch.equal(dqbuf[:, :C_], dq2)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. accumulate flags and strided forms of the reductions
@pytest.mark.parametrize("rows,c", [(1, 4), (7, 36), (65, 1024), (130, 160)])
def test_layer_norm_backward_accumulates(rows, c):
    """ln_bwd(acc_dx=True, acc_params=True), the only form the trainer uses: float64 autograd plus the prior contents, 3e-5."""
    from dsml_thesis_amd import ops, train_ops as T
    x = rnd(550, rows, c).double().requires_grad_(True)
    gamma = (1 + 0.1 * rnd(551, c)).double().requires_grad_(True)
    beta = (0.1 * rnd(552, c)).double().requires_grad_(True)
    dy = rnd(553, rows, c)
    F.layer_norm(x, (c,), gamma, beta, 1e-5).backward(dy.double())
    p_dx, p_dg, p_db = rnd(554, rows, c), rnd(555, c), rnd(556, c)
    xd, g32 = x.detach().float().cuda(), gamma.detach().float().cuda()
    stats = ops.ln_stats(xd)
    dx, dg, db = T.ln_bwd(dy.cuda(), xd, stats, g32, dx=p_dx.cuda(), acc_dx=True, dgamma=p_dg.cuda(), dbeta=p_db.cuda(), acc_params=True)
    _close(dx, x.grad + p_dx.double(), 3e-5, "ln dx accumulate")
    _close(dg, gamma.grad + p_dg.double(), 3e-5, "ln dgamma accumulate")
    _close(db, beta.grad + p_db.double(), 3e-5, "ln dbeta accumulate")
    # mixed flags: dx overwritten, parameters accumulated -- and the reverse
    dx, dg, db = T.ln_bwd(dy.cuda(), xd, stats, g32, dx=p_dx.cuda(), acc_dx=False, dgamma=p_dg.cuda(), dbeta=p_db.cuda(), acc_params=True)
    _close(dx, x.grad, 3e-5, "ln dx")
    _close(db, beta.grad + p_db.double(), 3e-5, "ln dbeta accumulate (dx plain)")
    dx, dg, db = T.ln_bwd(dy.cuda(), xd, stats, g32, dx=p_dx.cuda(), acc_dx=True, dgamma=p_dg.cuda(), dbeta=p_db.cuda(), acc_params=False)
    _close(dx, x.grad + p_dx.double(), 3e-5, "ln dx accumulate (params plain)")
    _close(dg, gamma.grad, 3e-5, "ln dgamma")


@pytest.mark.parametrize("c0,c1,hw", [(320, 160, 70), (32, 32, 1), (32, 32, 63), (32, 32, 65)])
def test_group_norm_backward_accumulates_both_sources(c0, c1, hw):
    """gn_bwd with acc0, acc1 and acc_params on, onto non-zero buffers; 320 + 160 channels give 15 channels per group, so one
    group straddles the two sources.  c0 = c1 = 32 has two channels per group: they are kept at least 1 apart (0.25-sigma noise
    around a 3-wide step), so that at hw = 1 the two-element group variance, and with it rstd, stays O(1).  Bound 5e-5 of
    max |ref|, as in test_group_norm_backward -- except dx at hw = 1: a group of two elements normalises to exactly +-1 whatever x
    is, so dx = sc dz - rstd (m1 + xhat m2) cancels to ~1e-6 of its terms (max |ref| 8e-6 against terms of O(1)) and no fp32
    evaluation can meet 5e-5 of the RESULT: fp32 torch autograd on the CPU misses it too (relative error 2.4e-2).  There the
    same 5e-5 is taken of max |sc dz|, the magnitude of the terms that cancel, which is what fp32 rounding scales with."""
    from dsml_thesis_amd import ops, train_ops as T, lib as L
    n, C = 2, c0 + c1
    step = 3.0 * (torch.arange(C) % 2).float()
    xall = rnd(560, n, hw, C) if c0 > 32 else 0.25 * rnd(560, n, hw, C) + step
    x0 = xall[..., :c0].contiguous().double().requires_grad_(True)
    x1 = xall[..., c0:].contiguous().double().requires_grad_(True)
    gamma = (1 + 0.1 * rnd(561, C)).double().requires_grad_(True)
    beta = (0.1 * rnd(562, C)).double().requires_grad_(True)
    xc = torch.cat([x0, x1], -1)
    z = F.group_norm(xc.permute(0, 2, 1), 32, gamma, beta, 1e-5).permute(0, 2, 1)
    z.retain_grad()
    dy = rnd(563, n, hw, C)
    F.silu(z).backward(dy.double())
    rstd = (xc.detach().view(n, hw, 32, C // 32).var((1, 3), unbiased=False) + 1e-5).rsqrt().repeat_interleave(C // 32, 1)   # [n][C]
    terms = (z.grad * gamma.detach() * rstd[:, None, :]).abs().max().item()
    dx_scale = {} if hw > 1 else {"dx0": terms / x0.grad.abs().max().item(), "dx1": terms / x1.grad.abs().max().item()}
    x0d, x1d, dyd = x0.detach().float().cuda(), x1.detach().float().cuda(), dy.cuda()
    g32, b32 = gamma.detach().float().cuda(), beta.detach().float().cuda()
    chunks = L.load().ldmk_gn_chunks(hw)
    partial = torch.empty(n * chunks * C * 3, device="cuda")
    coef = torch.empty(n, 2, C, device="cuda")
    ops.gn_coef(x0d, x1d, n, hw, g32, b32, 1e-5, partial=partial, coef=coef)
    mr = T.gn_group_stats(partial, c0, partial[n * chunks * c0 * 3:], c1, n, hw, 32, 1e-5)
    plain = T.gn_bwd(x0d, x1d, dyd, coef, mr, g32, n, hw)
    for got, ref, name in zip(plain, (x0.grad, x1.grad, gamma.grad, beta.grad), ("dx0", "dx1", "dgamma", "dbeta")):
        _close(got, ref, 5e-5 * dx_scale.get(name, 1.0), f"gn {name}")
    priors = [rnd(564, n, hw, c0), rnd(565, n, hw, c1), rnd(566, C), rnd(567, C)]
    acc = T.gn_bwd(x0d, x1d, dyd, coef, mr, g32, n, hw, dx0=priors[0].cuda(), acc0=True, dx1=priors[1].cuda(), acc1=True,
                   dgamma=priors[2].cuda(), dbeta=priors[3].cuda(), acc_params=True)
    for got, ref, pr, name in zip(acc, (x0.grad, x1.grad, gamma.grad, beta.grad), priors, ("dx0", "dx1", "dgamma", "dbeta")):
        _close(got, ref + pr.double(), 5e-5, f"gn {name} accumulate")            # the prior contents are O(1): the stated bound holds
    # one flag at a time: each source obeys its own flag
    only1 = T.gn_bwd(x0d, x1d, dyd, coef, mr, g32, n, hw, dx0=priors[0].cuda(), acc0=False, dx1=priors[1].cuda(), acc1=True)
    _close(only1[0], x0.grad, 5e-5 * dx_scale.get("dx0", 1.0), "gn dx0 (acc1 only)")
    _close(only1[1], x1.grad + priors[1].double(), 5e-5, "gn dx1 accumulate (acc1 only)")
    only0 = T.gn_bwd(x0d, x1d, dyd, coef, mr, g32, n, hw, dx0=priors[0].cuda(), acc0=True, dx1=priors[1].cuda(), acc1=False)
    _close(only0[0], x0.grad + priors[0].double(), 5e-5, "gn dx0 accumulate (acc0 only)")
    _close(only0[1], x1.grad, 5e-5 * dx_scale.get("dx1", 1.0), "gn dx1 (acc0 only)")
    again = T.gn_bwd(x0d, x1d, dyd, coef, mr, g32, n, hw)
    assert all(torch.equal(a, b) for a, b in zip(again, plain)), "the non-accumulating repeat must be bitwise the first call"


@pytest.mark.parametrize("rpg", [1, 255, 256, 257, 16385])
@pytest.mark.parametrize("N", [1, 63, 65, 160])
def test_colsum_strided_exact(N, rpg):
    """Column sums per row group with ldx > N on the input and the result in a column slice of a wider buffer (ldo > N), both
    accumulate settings; 16 385 rows per group are 64 splits with a ragged last one.  Integer data: exact."""
    from dsml_thesis_amd import train_ops as T
    groups = 3
    x = _ints(570, groups * rpg, N)
    ref = x.double().view(groups, rpg, N).sum(1)
    xbuf = torch.full((groups * rpg, N + 3), 3.0)
    xbuf[:, :N] = x
    xd = xbuf.cuda()[:, :N]
    for acc, fill in ((False, SENT), (True, 3.0)):
        obuf = torch.full((groups, N + 11), fill, device="cuda")
        T.colsum(xd, rows_per_group=rpg, out=obuf[:, 5:5 + N], accumulate=acc)
        _exact(obuf[:, 5:5 + N], ref + (fill if acc else 0.0), f"colsum accumulate={acc}")
        assert (obuf[:, :5] == fill).all() and (obuf[:, 5 + N:] == fill).all(), "colsum wrote outside its column slice"
    _exact(T.colsum(x.cuda(), rows_per_group=rpg), ref, "colsum, compact")


def test_mse_grad_with_padded_denominator():
    """denom != n (mean over the real elements of a channel-padded tensor) and more than one grid pass; 1e-6 as existing."""
    from dsml_thesis_amd import train_ops as T
    n = 256 * 256 * 3 + 5
    denom = 256 * 256 * 2 + 3
    pred, target = rnd(580, n), rnd(581, n)
    d = pred.double() - target.double()
    loss, dp = T.mse_grad(pred.cuda(), target.cuda(), denom=denom)
    _close(loss, (d * d).sum().view(1) / denom, 1e-6, "mse loss, denom != n")
    _close(dp, 2.0 * d / denom, 1e-6, "mse grad, denom != n")


@pytest.mark.parametrize("parts", [1, 3])
def test_head_permute_round_trip(parts):
    from dsml_thesis_amd import train_ops as T
    n, tokens, heads = 2, 5, 3
    src = rnd(590, n, tokens, parts, heads, 32)
    hm = T.head_permute(src.cuda(), n, tokens, parts, heads, True)
    assert torch.equal(hm.cpu().view(parts, n * heads, tokens, 32), src.permute(2, 0, 3, 1, 4).reshape(parts, n * heads, tokens, 32))
    back = T.head_permute(hm, n, tokens, parts, heads, False)
    assert torch.equal(back.cpu().view_as(src), src)


@pytest.mark.parametrize("cols", [1, 255, 257])
def test_softmax_backward_rows_edges(cols):
    from dsml_thesis_amd import train_ops as T
    s = rnd(600, 5, cols).double().requires_grad_(True)
    p = torch.softmax(s * 0.25, -1)
    dp = rnd(601, 5, cols)
    p.backward(dp.double())
    ds = T.softmax_bwd_rows_(p.detach().float().cuda(), dp.cuda().clone(), 0.25)
    if cols == 1:
        assert s.grad.abs().max().item() == 0.0 and ds.abs().max().item() <= 1e-7      # p == 1: p (dp - p dp) == 0
    else:
        _close(ds, s.grad, 2e-5, "softmax bwd")


@pytest.mark.parametrize("inner", [1, 3])
def test_geglu_backward_narrow(inner):
    from dsml_thesis_amd import train_ops as T
    pre = rnd(610, 7, 2 * inner).double().requires_grad_(True)
    v, g = pre.chunk(2, dim=-1)
    f = v * F.gelu(g)
    df = rnd(611, 7, inner)
    f.backward(df.double())
    pd = pre.detach().float().cuda()
    _close(T.geglu_fwd(pd), f.detach(), 1e-5, "geglu fwd")
    _close(T.geglu_bwd(pd, df.cuda()), pre.grad, 2e-5, "geglu bwd")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. rejections: refused on the host before any launch, outputs untouched
def test_wgrad_rejections(ops):
    from dsml_thesis_amd import train_ops as T
    from dsml_thesis_amd.lib import LdmkError
    a, dy = torch.ones(64, 448, device="cuda"), torch.ones(64, 64, device="cuda")
    dw, db = torch.full((448, 64), SENT, device="cuda"), torch.full((64,), SENT, device="cuda")
    ws = torch.full((4 * 449 * 64,), SENT, device="cuda")
    conv = (4, 4, 4, 4, 1, 1, 0)                                   # 64 rows = 4 samples of a 4x4 map

    def args(R=64, Kw=32, N=32, **kw):
        kw.setdefault("ws", ws)
        return T.wgrad_args(R, Kw, N, a, dy, dw, **kw)

    bad = {"N % 4": args(N=6, ldy=8, ldw=8), "Kw % 4": args(Kw=6, lda=8),
           "conv c = 48": args(Kw=432, c=48, conv=conv), "conv with batch = 2": args(R=32, Kw=288, c=32, conv=(4, 4, 4, 4, 1, 1, 0), batch=2),
           "dbias with batch = 2": args(R=32, batch=2, a_bstride=32 * 32, dy_bstride=32 * 32, dw_bstride=32 * 32, dbias=db),
           "splitr = 257": args(splitr=257), "lda < Kw": args(lda=28)}
    short = args(splitr=2)
    short.ws_elems = 2 * 32 * 32 - 1                               # one float less than two [Kw][N] slabs
    bad["workspace one float short"] = short
    short_b = args(splitr=2, dbias=db)
    short_b.ws_elems = 2 * 33 * 32 - 1                             # ... and than two slabs with their bias row
    bad["workspace one float short (bias row)"] = short_b
    for what, w in bad.items():
        with pytest.raises(LdmkError):
            T.wgrad(w)
        assert (dw == SENT).all() and (db == SENT).all() and (ws == SENT).all(), f"{what}: refused, but memory was written"
    ok = args(splitr=2)                                            # the same call with the workspace it needs goes through
    ok.ws_elems = 2 * 32 * 32
    T.wgrad(ok)
    assert (dw.view(-1)[:32 * 32] == 64.0).all() and (dw.view(-1)[32 * 32:] == SENT).all()      # compact [32][32], 64 rows of ones


@pytest.mark.parametrize("c", [1028, 6])
def test_ln_bwd_rejects_unsupported_widths(c):
    from dsml_thesis_amd import train_ops as T
    from dsml_thesis_amd.lib import LdmkError
    x, dy = torch.ones(4, c, device="cuda"), torch.ones(4, c, device="cuda")
    stats, gamma = torch.ones(4, 2, device="cuda"), torch.ones(c, device="cuda")
    dx, dg, db = (torch.full(s, SENT, device="cuda") for s in ((4, c), (c,), (c,)))
    with pytest.raises(LdmkError):
        T.ln_bwd(dy, x, stats, gamma, dx=dx, dgamma=dg, dbeta=db)
    assert (dx == SENT).all() and (dg == SENT).all() and (db == SENT).all()


def test_attn_cross_bwd_rejects_long_context():
    from dsml_thesis_amd import train_ops as T
    from dsml_thesis_amd.lib import LdmkError
    n, tokens, L_ctx, heads = 1, 4, 129, 1
    q, dout = torch.ones(tokens, 32, device="cuda"), torch.ones(tokens, 32, device="cuda")
    k, v = torch.ones(L_ctx, 32, device="cuda"), torch.ones(L_ctx, 32, device="cuda")
    dq, dk, dv = (torch.full(s, SENT, device="cuda") for s in ((tokens, 32), (L_ctx, 32), (L_ctx, 32)))
    with pytest.raises(LdmkError, match="ctx_len"):
        T.attn_cross_bwd(q, k, v, dout, n, tokens, L_ctx, heads, dq=dq, dk=dk, dv=dv)
    assert (dq == SENT).all() and (dk == SENT).all() and (dv == SENT).all()
