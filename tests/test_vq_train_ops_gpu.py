"""GPU: the kernels of first-stage (VQGAN) training (csrc/vq_train.hip) and the asymmetric-pad stride-2 data gradient, each
against float64 from the same fp32 operands, at the smallest shapes that can go wrong.

Bounds.  Reductions (quantiser loss, dE, dW, db): the torch fp32 formulation (index_add_ / sum / einsum on the GPU) is
measured here against the same float64 reference and the kernel gets twice that, with a floor of 2^-23 of max |ref| -- the
rule of test_kl_first_stage_gpu.py::test_gauss_posterior_against_float64.  Both figures are printed.  Elementwise outputs
have bounds from the number format, stated where they are used."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rnd

pytestmark = pytest.mark.gpu

BETA, W = 0.25, 0.75            # exact in fp32: the kernel and the float64 reference see the same operands


@pytest.fixture(scope="module")
def T():
    from dsml_thesis_amd import lib, train_ops
    lib.load()
    return train_ops


def _maxerr(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item()


def _reduction_ok(what, got, torch32, ref):
    """kernel error <= max(2 x the torch fp32 formulation's error, 2^-23 max|ref|), errors as max abs against float64"""
    k, t = _maxerr(got, ref), _maxerr(torch32, ref)
    bound = max(2.0 * t, 2.0 ** -23 * ref.abs().max().item())
    print(f"{what}: kernel {k:.3e} / torch fp32 {t:.3e} / bound {bound:.3e} (max |ref| {ref.abs().max().item():.3e})")
    assert k <= bound, f"{what}: {k:.3e} > {bound:.3e}"


# ------------------------------------------------------------------------------------------ quantiser loss and gradients
VQ_CASES = [(1, 1, 1, 3, 1, False),          # one row, one code
            (2, 5, 7, 3, 7, False),          # scalar kernel (hw % 4 != 0), ragged 64-row step, codes < one tile
            (2, 16, 16, 4, 64, False),       # dim 4, 16-byte kernel, exactly one code tile
            (1, 32, 32, 3, 16384, False),    # 256 code tiles, nearly every code unused
            (2, 5, 7, 3, 7, True),           # a hand-made idx: every row goes to one code
            (2, 24, 48, 4, 100, False),      # 2304 rows: every wave of a tile has more than one 64-row step; ragged code tile
            (16, 32, 32, 3, 16384, False)]   # 16 x 1024 rows against 16384 codes: the shipped VQ-f4 training shape


@pytest.mark.parametrize("n,h,w,dim,n_e,one_code", VQ_CASES, ids=lambda v: str(v))
def test_vq_loss_and_gradients_against_float64(T, n, h, w, dim, n_e, one_code):
    from dsml_thesis_amd import ops
    hw = h * w
    z = (rnd(700 + n_e, n, dim, h, w) * 0.7).cuda()
    cb = rnd(701 + n_e, n_e, dim).cuda()
    if one_code:
        idx = torch.full((n * hw,), 3, dtype=torch.int32, device="cuda")
    else:                            # the kernel's own choice: the case does not depend on which of two near-tied codes wins
        idx = ops.vq_nearest(z, cb)[1].reshape(-1).contiguous()
    assert idx.dtype == torch.int32 and idx.numel() == n * hw
    dzq = rnd(702 + n_e, n, dim, h, w).cuda()
    N = n * hw * dim
    z64, cb64, il = z.double().cpu(), cb.double().cpu(), idx.long().cpu()
    e64 = cb64[il].view(n, h, w, dim).permute(0, 3, 1, 2)
    diff = z64 - e64
    m = (diff * diff).sum() / N
    loss_ref = (m + BETA * m).view(1)
    rows_ref = (e64 - z64).permute(0, 2, 3, 1).reshape(n * hw, dim)
    cnt_ref = torch.bincount(il, minlength=n_e)
    # the torch fp32 formulation, on the GPU
    e32 = cb[idx.long()].view(n, h, w, dim).permute(0, 3, 1, 2)
    loss32 = (((e32 - z) ** 2).mean() * (1.0 + BETA)).view(1)
    rows32 = (e32 - z).permute(0, 2, 3, 1).reshape(n * hw, dim)
    for legacy in (True, False):
        cz, ce = (1.0, BETA) if legacy else (BETA, 1.0)
        dE_ref = torch.zeros(n_e, dim, dtype=torch.float64).index_add_(0, il, rows_ref) * (W * ce * 2.0 / N)
        dE32 = torch.zeros(n_e, dim, device="cuda").index_add_(0, idx.long(), rows32) * (W * ce * 2.0 / N)
        dE, cnt = T.vq_codebook_grad(z, cb, idx, beta=BETA, legacy=legacy, w=W)
        assert torch.equal(cnt.cpu().long(), cnt_ref), "count == bincount"
        assert (dE[cnt == 0] == 0).all(), "unused codes: exact zero rows"
        _reduction_ok(f"dE legacy={legacy}", dE, dE32, dE_ref)
        dE2, cnt2 = T.vq_codebook_grad(z, cb, idx, beta=BETA, legacy=legacy, w=W)
        assert torch.equal(dE, dE2) and torch.equal(cnt, cnt2), "two calls, identical bits"
        for g in (dzq, None):
            loss, dz = T.vq_loss_bwd(z, cb, idx, dzq=g, beta=BETA, legacy=legacy, w=W)
            _reduction_ok(f"loss legacy={legacy} dzq={'yes' if g is not None else 'no'}", loss, loss32, loss_ref)
            dz_ref = (0.0 if g is None else g.double().cpu()) + (W * cz * 2.0 / N) * diff
            err = (dz.double().cpu() - dz_ref).abs()
            assert (err <= 1e-6 * dz_ref.abs()).all(), f"dz: elementwise rtol 1e-6, worst {(err / dz_ref.abs().clamp_min(1e-300)).max():.3e}"
            loss2, dz2 = T.vq_loss_bwd(z, cb, idx, dzq=g, beta=BETA, legacy=legacy, w=W)
            assert torch.equal(loss, loss2) and torch.equal(dz, dz2), "two calls, identical bits"
        only, none = T.vq_loss_bwd(z, cb, idx, beta=BETA, legacy=legacy, w=W, want_dz=False)
        assert none is None and torch.equal(only, loss), "loss alone (validation step)"
    if n_e == 16384:
        assert (cnt_ref == 0).sum() >= n_e - n * hw, "nearly every code unused"
    if one_code:
        assert cnt_ref[3] == n * hw and (cnt_ref > 0).sum() == 1
    # an unaligned base pointer takes the scalar kernel: dz agrees bit for bit, the loss (another summation order) to its bound
    flat = torch.empty(z.numel() + 1, device="cuda")
    flat[1:].copy_(z.flatten())
    loss3, dz3 = T.vq_loss_bwd(flat[1:].view_as(z), cb, idx, beta=BETA, legacy=False, w=W)
    assert torch.equal(dz3, dz)
    _reduction_ok("loss, scalar kernel", loss3, loss32, loss_ref)


# ------------------------------------------------------------------------------------------ 1x1 NCHW backward
@pytest.mark.parametrize("n,h,w,cin,cout", [(1, 1, 1, 3, 3), (2, 5, 7, 3, 4), (1, 64, 64, 4, 4), (2, 32, 32, 8, 8)], ids=lambda v: str(v))
def test_conv1x1_nchw_backward_against_float64(T, n, h, w, cin, cout):
    """(n, hw, cin, cout) = (1, 1, 3, 3), (2, 35, 3, 4), (1, 4096, 4, 4), (2, 1024, 8, 8).  dx is a fused multiply-add chain
    of cout terms per element: |err| <= cout 2^-24 (|W|^T |dy|)."""
    x, dy, wt = rnd(710, n, cin, h, w).cuda(), rnd(711, n, cout, h, w).cuda(), (rnd(712, cout, cin) * 0.5).cuda()
    x64, dy64, w64 = x.double().cpu(), dy.double().cpu(), wt.double().cpu()
    dx_ref = torch.einsum("oc,nohw->nchw", w64, dy64)
    dw_ref = torch.einsum("nohw,nchw->oc", dy64, x64)
    db_ref = dy64.sum((0, 2, 3))
    dx, dw, db = T.conv1x1_nchw_bwd(x, dy, wt.view(cout, cin, 1, 1))
    bound = cout * 2.0 ** -24 * torch.einsum("oc,nohw->nchw", w64.abs(), dy64.abs())
    assert ((dx.double().cpu() - dx_ref).abs() <= bound).all(), "dx"
    _reduction_ok("dW", dw, torch.einsum("nohw,nchw->oc", dy, x), dw_ref)
    _reduction_ok("db", db, dy.sum((0, 2, 3)), db_ref)
    dx2, dw2, db2 = T.conv1x1_nchw_bwd(x, dy, wt)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2), "two calls, identical bits"
    # accumulate: one fp32 add onto what is there; dx not requested
    dwa, dba = torch.full_like(dw, 3.0), torch.full_like(db, -2.0)
    none, _, _ = T.conv1x1_nchw_bwd(x, dy, wt, dw=dwa, db=dba, accumulate=True, want_dx=False)
    assert none is None and torch.equal(dwa, dw + 3.0) and torch.equal(dba, db - 2.0)


# ------------------------------------------------------------------------------------------ L1 pixel loss
def test_l1_grad_with_ties_and_padded_denominator(T):
    """denom != n and more than one grid pass, as test_mse_grad_with_padded_denominator; every 7th element is an exact tie.
    dpred is sign / denom rounded once.  The loss sums |fl(pred - target)|: the subtraction's rounding (2^-24 of each term,
    all of one sign) plus the final rounding bound it by 2^-23 of the sum."""
    n = 256 * 256 * 3 + 5
    denom = 256 * 256 * 2 + 3
    pred, target = rnd(720, n), rnd(721, n)
    target[::7] = pred[::7]
    d = pred.double() - target.double()
    assert (d == 0).sum() >= n // 7 and (d > 0).any() and (d < 0).any()
    loss, dp = T.l1_grad(pred.cuda(), target.cuda(), denom=denom)
    ref = d.abs().sum() / denom
    err = abs(loss.double().cpu().item() - ref.item())
    print(f"l1 loss: kernel {err:.3e} / bound {2.0 ** -23 * ref.item():.3e}")
    assert err <= 2.0 ** -23 * ref.item()
    assert torch.equal(dp.cpu(), (torch.sign(d) / denom).float()), "dpred = sign / denom; sign(0) = 0"
    assert (dp.cpu()[::7] == 0).all()
    loss_n, dp_n = T.l1_grad(pred.cuda(), target.cuda())
    assert abs(loss_n.double().cpu().item() - d.abs().mean().item()) <= 2.0 ** -23 * d.abs().mean().item()
    assert torch.equal(dp_n.cpu(), (torch.sign(d) / n).float())


# ------------------------------------------------------------------------------------------ asymmetric stride-2 data gradient
def _close(got, ref, rtol, what):           # the bound form of tests/test_backward_gpu.py
    ref = ref.to(torch.float64)
    err = (got.detach().cpu().to(torch.float64) - ref).abs().max().item()
    bound = rtol * max(ref.abs().max().item(), 1e-30)
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


@pytest.mark.parametrize("n,h,w,cin,cout", [(1, 4, 4, 32, 32), (2, 6, 10, 32, 64), (1, 5, 7, 64, 32)], ids=lambda v: str(v))
def test_downsample_conv_data_gradient(T, n, h, w, cin, cout):
    """Encoder Downsample: F.pad(x, (0,1,0,1)) then a stride-2 pad-0 convolution; 3e-5 of max |ref|, the bound
    tests/test_backward_gpu.py::test_conv3x3_backward holds the pad-1 form to."""
    from dsml_thesis_amd import ops
    with torch.enable_grad():
        x = rnd(730, n, cin, h, w).double().requires_grad_(True)
        wt = (rnd(731, cout, cin, 3, 3) / np.sqrt(9 * cin)).double()
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, None, stride=2)
        dy = rnd(732, *y.shape)
        y.backward(dy.double())
    assert y.shape[2:] == ((h + 1 - 3) // 2 + 1, (w + 1 - 3) // 2 + 1)
    dyd = dy.permute(0, 2, 3, 1).contiguous().cuda()
    wd = T.pack_dgrad3x3(ops.pack_conv3x3(wt.float().cuda()), cin, cout)
    dx = T.conv3x3_dgrad(dyd, wd, (h, w), stride=2, pad_lo=0)
    _close(dx.permute(0, 3, 1, 2), x.grad, 3e-5, "downsample conv dgrad")


@pytest.mark.parametrize("stride", [1, 2])
def test_dgrad_pad_lo_1_is_the_old_call(T, stride):
    """The default path against the argument block conv3x3_dgrad built before it had the keyword (written out by hand here:
    tap origin 1, dy zero-inserted for stride 2), bit for bit."""
    from dsml_thesis_amd import ops
    n, h, cin, cout = 2, 6, 64, 32
    oh = (h + 2 - 3) // stride + 1
    dyd = rnd(740, n, oh, oh, cout).cuda()
    wd = T.pack_dgrad3x3(ops.pack_conv3x3((rnd(741, cout, cin, 3, 3) / 24.0).cuda()), cin, cout)
    old = torch.empty(n, h, h, cin, device="cuda")
    a = ops.make_igemm_args(n * h * h, cin, 9 * cout, dyd, cout, wd, old, cin, h * h, compute=T.COMPUTE,
                            conv=(oh, oh, h, h, 1, 1, 2 if stride == 2 else 0))
    ops.igemm(a)
    assert torch.equal(T.conv3x3_dgrad(dyd, wd, (h, h), stride=stride), old), "default keyword"
    assert torch.equal(T.conv3x3_dgrad(dyd, wd, (h, h), stride=stride, pad_lo=1), old), "pad_lo=1"
