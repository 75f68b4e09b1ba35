"""Tensor-level wrappers of the training-step kernels (include/ldmk.h, section "Training step").
CUDA tensors only; every call goes to libldmk.so -- there is no PyTorch fallback."""
import ctypes as C

import torch

from . import lib as L
from . import ops
from .ops import _ptr, stream


def _f32(*shape, device="cuda"):
    return torch.empty(*shape, device=device, dtype=torch.float32)


# Arithmetic of the matrix-core GEMMs the training helpers below launch: L.COMPUTE_F32 (parity path) or L.COMPUTE_BF16
# (BASELINE configs[4]: bf16 operands, fp32 accumulation / master weights).  UNetTrainer sets it from its `compute` argument
# at the start of every forward / backward; the step is single-threaded host code.
COMPUTE = L.COMPUTE_F32


def set_compute(mode):
    global COMPUTE
    COMPUTE = {None: L.COMPUTE_F32, "f32": L.COMPUTE_F32, "fp32": L.COMPUTE_F32, "bf16": L.COMPUTE_BF16}.get(mode, mode)
    return COMPUTE


def wgrad_args(R, Kw, N, a, dy, dw, c=0, lda=None, conv=None, ldy=None, ldw=None, accumulate=False, alpha=1.0, batch=1,
               a_bstride=0, dy_bstride=0, dw_bstride=0, splitr=0, ws=None, dbias=None):
    w = L.WgradArgs()
    w.R, w.Kw, w.N = R, Kw, N
    w.a, w.dy, w.dw = _ptr(a), _ptr(dy), _ptr(dw)
    w.c = c or Kw
    if conv is not None:
        w.a_mode = L.A_CONV3X3
        w.in_h, w.in_w, w.out_h, w.out_w, w.stride, w.pad_lo, w.upsample = conv
        w.lda = w.c
    else:
        w.a_mode = L.A_ROWS
        w.lda = lda if lda is not None else Kw
        w.out_h, w.out_w = 1, 1
    w.ldy = ldy if ldy is not None else N
    w.ldw = ldw if ldw is not None else N
    w.accumulate, w.alpha = 1 if accumulate else 0, alpha
    w.batch, w.a_bstride, w.dy_bstride, w.dw_bstride = batch, a_bstride, dy_bstride, dw_bstride
    w.splitr = splitr
    w.dbias = _ptr(dbias)
    w.compute = COMPUTE
    if ws is not None:
        w.ws, w.ws_elems = ws.data_ptr(), ws.numel()
    return w


def wgrad_workspace_elems(w):
    sr = C.c_int(0)
    L.call("ldmk_wgrad_plan", C.byref(w), C.byref(sr))
    return sr.value, (sr.value * max(1, w.batch) * (w.Kw + (1 if w.dbias else 0)) * w.N if sr.value > 1 else 0)


def wgrad(w):
    L.call("ldmk_wgrad", C.byref(w), stream())


_WS = {}
_WS_RETIRED = []     # outgrown scratches stay alive: a captured hipGraph may still replay partial sums into them


def _workspace(dev, elems):
    """One scratch per device for the wgrad partial slabs (stream-ordered reuse).  It only grows outside a stream
    capture, geometrically (so the retired ones add up to less than the live one), and an outgrown scratch is never
    freed: hipGraphs captured earlier keep its address."""
    ws = _WS.get(dev)
    if ws is None or ws.numel() < elems:
        if torch.cuda.is_current_stream_capturing():
            raise L.LdmkError(f"wgrad scratch of {elems} floats requested during a stream capture, but only "
                              f"{0 if ws is None else ws.numel()} are allocated: run the step once eagerly first")
        if ws is not None:
            _WS_RETIRED.append(ws)
        ws = _f32(max(int(elems), 1 << 22, 0 if ws is None else 2 * ws.numel()), device=dev)
        _WS[dev] = ws
    return ws


def wgrad_linear(a2d, dy2d, dw=None, accumulate=False, lda=None, splitr=0, dbias=None):
    """dW[K][N] = a2d[R][K]^T @ dy2d[R][N]  (+ dbias[N] = column sums of dy2d)."""
    R, K = a2d.shape
    N = dy2d.shape[1]
    if dw is None:
        dw = _f32(K, N, device=a2d.device)
    w = wgrad_args(R, K, N, a2d, dy2d, dw, lda=lda if lda is not None else a2d.stride(0), ldy=dy2d.stride(0),
                   accumulate=accumulate, splitr=splitr, dbias=dbias)
    sr, need = wgrad_workspace_elems(w) if splitr == 0 else (splitr, splitr * (K + 1) * N)
    ws = _workspace(a2d.device, need)
    w.splitr, w.ws, w.ws_elems = sr, ws.data_ptr(), ws.numel()
    wgrad(w)
    return dw


def wgrad_conv3x3(x, dy, stride=1, pad_lo=1, upsample=False, dw=None, accumulate=False, dbias=None):
    """x: (n,h,w,c) NHWC input the forward conv consumed, dy: (n,oh,ow,cout) -> packed dW [9c][cout]."""
    n, h, w_, c = x.shape
    _, oh, ow, cout = dy.shape
    if dw is None:
        dw = _f32(9 * c, cout, device=x.device)
    w = wgrad_args(n * oh * ow, 9 * c, cout, x, dy, dw, c=c, conv=(h, w_, oh, ow, stride, pad_lo, 1 if upsample else 0),
                   accumulate=accumulate, dbias=dbias)
    sr, need = wgrad_workspace_elems(w)
    ws = _workspace(x.device, need)
    w.splitr, w.ws, w.ws_elems = sr, ws.data_ptr(), ws.numel()
    wgrad(w)
    return dw


def pack_dgrad3x3(wp, cin, cout, out=None):
    if out is None:
        out = _f32(9 * cout, cin, device=wp.device)
    L.call("ldmk_pack_dgrad3x3", _ptr(wp), _ptr(out), cin, cout, stream())
    return out


def conv3x3_dgrad(dy, wd, in_hw, stride=1, out=None, residual=None, pad_lo=1, compute=None, splitk_ws=None):
    """Data gradient of a 3x3 convolution: dy (n,oh,ow,cout), wd = pack_dgrad3x3 weights [9*cout][cin] ->
    (n,h,w,cin).  stride 2 reads dy zero-inserted (ldmk_igemm upsample=2).  pad_lo is the FORWARD convolution's: 1 is the
    pad-1 form; 0 with stride 2 is the encoder's Downsample, F.pad(x, (0,1,0,1)) then a pad-0 convolution (model.py:72-76).
    With the taps mirrored, input pixel i reads the zero-inserted dy at i - (2 - pad_lo) + tap, so the transposed
    convolution's own pad_lo is 2 - pad_lo."""
    n, oh, ow, cout = dy.shape
    h, w_ = in_hw
    cin = wd.shape[1]
    if pad_lo not in (0, 1) or (pad_lo == 0 and stride != 2):
        raise ValueError(f"conv3x3_dgrad: pad_lo={pad_lo}, stride={stride}: pad_lo is 1, or 0 with stride 2")
    if out is None:
        out = _f32(n, h, w_, cin, device=dy.device)
    a = ops.make_igemm_args(n * h * w_, cin, 9 * cout, dy, cout, wd, out, cin, h * w_, compute=COMPUTE if compute is None else compute,
                            conv=(oh, ow, h, w_, 1, 2 - pad_lo, 2 if stride == 2 else 0), residual=residual, splitk_ws=splitk_ws)
    ops.igemm(a)
    return out


def gn_group_stats(partial0, c0, partial1, c1, n, hw, groups, eps, out=None):
    if out is None:
        out = _f32(n, groups, 2, device=partial0.device)
    L.call("ldmk_gn_group_stats", _ptr(partial0), c0, _ptr(partial1), c1, n, hw, groups, eps, _ptr(out), stream())
    return out


def gn_bwd(x0, x1, dy, coef, mr, gamma, n, hw, groups=32, silu=True, dx0=None, acc0=False, dx1=None, acc1=False,
           dgamma=None, dbeta=None, acc_params=False):
    c0 = x0.shape[-1]
    c1 = 0 if x1 is None else x1.shape[-1]
    Cc = c0 + c1
    dev = x0.device
    dx0 = torch.empty_like(x0) if dx0 is None else dx0
    if x1 is not None and dx1 is None:
        dx1 = torch.empty_like(x1)
    dgamma = _f32(Cc, device=dev) if dgamma is None else dgamma
    dbeta = _f32(Cc, device=dev) if dbeta is None else dbeta
    scratch = _f32(L.load().ldmk_gn_bwd_scratch_elems(n, hw, Cc, groups), device=dev)
    L.call("ldmk_gn_bwd", _ptr(x0), c0, _ptr(x1), c1, _ptr(dy), _ptr(coef), _ptr(mr), _ptr(gamma), n, hw, groups,
           1 if silu else 0, _ptr(dx0), 1 if acc0 else 0, _ptr(dx1), 1 if acc1 else 0, _ptr(dgamma), _ptr(dbeta),
           1 if acc_params else 0, _ptr(scratch), stream())
    return dx0, dx1, dgamma, dbeta


def gn_coef_film_(coef, film):
    """Fold FiLM into GroupNorm coefficient planes in place: coef [n][2][C], film = the sample rows (scale | shift), [n][>= 2C]."""
    n, _, c = coef.shape
    L.call("ldmk_gn_coef_film", _ptr(coef), _ptr(film), film.stride(0), n, c, stream())
    return coef


def gn_film_bwd(x, dy, coef, mr, gamma, beta, film, n, hw, dfilm, groups=32, dx=None, acc_dx=False, dgamma=None, dbeta=None,
                acc_params=False):
    """Backward of h = SiLU(GroupNorm(x) (1 + scale) + shift): `coef` are the FiLM-folded planes the forward applied, `film` /
    `dfilm` the [n][>= 2C] (scale | shift) rows and their gradient (column slices of emb_all / d_emb_all)."""
    c = x.shape[-1]
    dev = x.device
    dx = torch.empty_like(x) if dx is None else dx
    dgamma = _f32(c, device=dev) if dgamma is None else dgamma
    dbeta = _f32(c, device=dev) if dbeta is None else dbeta
    scratch = _f32(L.load().ldmk_gn_film_bwd_scratch_elems(n, hw, c), device=dev)
    L.call("ldmk_gn_film_bwd", _ptr(x), _ptr(dy), _ptr(coef), _ptr(mr), _ptr(gamma), _ptr(beta), _ptr(film), film.stride(0), n, hw, c,
           groups, _ptr(dx), 1 if acc_dx else 0, _ptr(dgamma), _ptr(dbeta), 1 if acc_params else 0, _ptr(dfilm), dfilm.stride(0),
           _ptr(scratch), stream())
    return dx, dgamma, dbeta


def label_emb_bwd(d_emb, y, dw, accumulate=False):
    """dw[y[i]] (+)= d_emb[i]: d_emb [n][emb] fp32, y [n] int64, dw [classes][emb]."""
    n, emb = d_emb.shape
    L.call("ldmk_label_emb_bwd", _ptr(d_emb), _ptr(y), n, emb, dw.shape[0], _ptr(dw), 1 if accumulate else 0, stream())
    return dw


def ln_apply(x2d, stats, gamma, beta, out=None):
    rows, c = x2d.shape
    out = torch.empty_like(x2d) if out is None else out
    L.call("ldmk_ln_apply", _ptr(x2d), _ptr(stats), _ptr(gamma), _ptr(beta), _ptr(out), rows, c, stream())
    return out


def ln_bwd(dy, x2d, stats, gamma, dx=None, acc_dx=False, dgamma=None, dbeta=None, acc_params=False):
    rows, c = x2d.shape
    dev = x2d.device
    dx = torch.empty_like(x2d) if dx is None else dx
    dgamma = _f32(c, device=dev) if dgamma is None else dgamma
    dbeta = _f32(c, device=dev) if dbeta is None else dbeta
    scratch = _f32(L.load().ldmk_ln_bwd_blocks(rows) * c * 2, device=dev)
    L.call("ldmk_ln_bwd", _ptr(dy), _ptr(x2d), _ptr(stats), _ptr(gamma), _ptr(dx), 1 if acc_dx else 0, rows, c, _ptr(dgamma),
           _ptr(dbeta), 1 if acc_params else 0, _ptr(scratch), stream())
    return dx, dgamma, dbeta


def geglu_fwd(pre, out=None):
    rows, two = pre.shape
    out = _f32(rows, two // 2, device=pre.device) if out is None else out
    L.call("ldmk_geglu_fwd", _ptr(pre), _ptr(out), rows, two // 2, stream())
    return out


def geglu_bwd(pre, df, out=None):
    rows, two = pre.shape
    out = torch.empty_like(pre) if out is None else out
    L.call("ldmk_geglu_bwd", _ptr(pre), _ptr(df), _ptr(out), rows, two // 2, stream())
    return out


def softmax_bwd_rows_(p2d, dp2d, scale=1.0):
    rows, cols = p2d.shape
    L.call("ldmk_softmax_bwd_rows", _ptr(p2d), _ptr(dp2d), rows, cols, scale, stream())
    return dp2d


def colsum(x2d, rows_per_group=None, out=None, accumulate=False):
    rows, n = x2d.shape
    rpg = rows if rows_per_group is None else rows_per_group
    groups = rows // rpg
    out = _f32(groups, n, device=x2d.device) if out is None else out
    scratch = _f32(groups * L.load().ldmk_colsum_splits(rpg) * n, device=x2d.device)
    L.call("ldmk_colsum", _ptr(x2d), x2d.stride(0), rpg, groups, n, _ptr(out), out.stride(0) if out.dim() > 1 else n,
           1 if accumulate else 0, _ptr(scratch), stream())
    return out


def sumpool2(du, out=None, accumulate=False):
    n, h2, w2, c = du.shape
    out = _f32(n, h2 // 2, w2 // 2, c, device=du.device) if out is None else out
    L.call("ldmk_sumpool2", _ptr(du), _ptr(out), n, h2 // 2, w2 // 2, c, 1 if accumulate else 0, stream())
    return out


def resample2(x, up):
    """The parameter-free resampling of a ResBlock(up=True / down=True), NHWC: nearest x2 or avg_pool2d(2, 2)."""
    n, h, w, c = x.shape
    oh, ow = (2 * h, 2 * w) if up else (h // 2, w // 2)
    out = _f32(n, oh, ow, c, device=x.device)
    L.call("ldmk_resample2", _ptr(x), _ptr(out), n, min(h, oh), min(w, ow), c, 1 if up else 0, stream())
    return out


def avgpool2_bwd(dy, out=None, accumulate=False):
    """avg_pool2d(2, 2) backward: dy (n,h,w,c) -> (n,2h,2w,c), every input pixel gets a quarter of its output pixel's gradient."""
    n, h, w, c = dy.shape
    out = _f32(n, 2 * h, 2 * w, c, device=dy.device) if out is None else out
    L.call("ldmk_avgpool2_bwd", _ptr(dy), _ptr(out), n, h, w, c, 1 if accumulate else 0, stream())
    return out


def silu(x, out=None):
    out = torch.empty_like(x) if out is None else out
    L.call("ldmk_silu", _ptr(x), _ptr(out), x.numel(), stream())
    return out


def silu_bwd(x, dy, out=None):
    out = torch.empty_like(x) if out is None else out
    L.call("ldmk_silu_bwd", _ptr(x), _ptr(dy), _ptr(out), x.numel(), stream())
    return out


def axpy_(y, x, a=1.0):
    L.call("ldmk_axpy", _ptr(y), _ptr(x), a, y.numel(), stream())
    return y


def q_sample(x0, noise, t, sqrt_ac, sqrt_1mac, out=None):
    out = torch.empty_like(x0) if out is None else out
    L.call("ldmk_q_sample", _ptr(x0), _ptr(noise), _ptr(t), _ptr(sqrt_ac), _ptr(sqrt_1mac), _ptr(out), x0.shape[0],
           x0[0].numel(), stream())
    return out


def mse_grad(pred, target, dpred=None, loss=None, denom=0):
    dpred = torch.empty_like(pred) if dpred is None else dpred
    loss = _f32(1, device=pred.device) if loss is None else loss
    scratch = torch.empty(256, device=pred.device, dtype=torch.float64)
    L.call("ldmk_mse_grad", _ptr(pred), _ptr(target), _ptr(dpred), pred.numel(), denom, _ptr(loss), _ptr(scratch), stream())
    return loss, dpred


def l1_grad(pred, target, dpred=None, loss=None, denom=0):
    """loss = mean|pred - target|, dpred = sign(pred - target) / denom (sign(0) = 0); the sibling of mse_grad."""
    ops._chk(pred, "l1_grad pred")
    ops._chk(target, "l1_grad target")
    if target.numel() != pred.numel():
        raise ValueError(f"l1_grad: pred {tuple(pred.shape)} against target {tuple(target.shape)}")
    dpred = torch.empty_like(pred) if dpred is None else dpred
    loss = _f32(1, device=pred.device) if loss is None else loss
    scratch = torch.empty(256, device=pred.device, dtype=torch.float64)
    L.call("ldmk_l1_grad", _ptr(pred), _ptr(target), _ptr(dpred), pred.numel(), denom, _ptr(loss), _ptr(scratch), stream())
    return loss, dpred


LOSS_TYPES = {"l1": 1, "l2": 2}


def diffusion_loss(pred_pad, target, t, logvar, lvlb_weights, loss_type="l2", l_simple_weight=1.0, original_elbo_weight=0.0,
                   want_dpred=True, want_dlogvar=True, dpred=None):
    """The full objective of p_losses (ddpm.py:1014-1047) in one launch pair (ldmk_diffusion_loss): pred_pad (n,H,W,32) or
    (n,H*W,32) channel-padded NHWC, target (n,c,H,W) NCHW read in place, t (n,) int64, logvar / lvlb_weights (T,).
    -> dict(scalars=[loss, loss_simple, loss_gamma, loss_vlb] (4,), ls (n,), dpred like pred_pad or None, dlogvar (T,) or None)."""
    for name, x in (("pred", pred_pad), ("target", target), ("logvar", logvar), ("lvlb_weights", lvlb_weights), ("dpred", dpred)):
        ops._chk(x, f"diffusion_loss {name}")
    if not (t.is_cuda and t.is_contiguous()):
        raise L.LdmkError("diffusion_loss t: expected a contiguous CUDA tensor")
    if loss_type not in LOSS_TYPES:
        raise NotImplementedError(f"unknown loss type '{loss_type}'")
    n, c = target.shape[0], target.shape[1]
    hw = target[0, 0].numel()
    T_ = logvar.numel()
    if pred_pad.shape[-1] != 32 or pred_pad.numel() != n * hw * 32 or t.dtype != torch.int64 or t.numel() != n \
            or lvlb_weights.numel() != T_ or logvar.dtype != torch.float32 or lvlb_weights.dtype != torch.float32 \
            or pred_pad.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError(f"diffusion_loss: pred {tuple(pred_pad.shape)} {pred_pad.dtype}, target {tuple(target.shape)} {target.dtype}, "
                         f"t {tuple(t.shape)} {t.dtype}, logvar {tuple(logvar.shape)}, lvlb_weights {tuple(lvlb_weights.shape)}")
    dev = pred_pad.device
    if want_dpred and dpred is None:
        dpred = torch.empty_like(pred_pad)
    elif not want_dpred:
        dpred = None
    if dpred is not None and (dpred.shape != pred_pad.shape or dpred.dtype != torch.float32):
        raise ValueError(f"diffusion_loss: dpred {tuple(dpred.shape)} against pred {tuple(pred_pad.shape)}")
    dlogvar = _f32(T_, device=dev) if want_dlogvar else None
    scalars, ls = _f32(4, device=dev), _f32(n, device=dev)
    scratch = torch.empty(L.load().ldmk_diffusion_loss_scratch_elems(n), device=dev, dtype=torch.float64)
    L.call("ldmk_diffusion_loss", _ptr(pred_pad), _ptr(target), _ptr(t), _ptr(logvar), _ptr(lvlb_weights), _ptr(dpred), _ptr(dlogvar),
           _ptr(scalars), _ptr(ls), n, c, hw, T_, LOSS_TYPES[loss_type], float(l_simple_weight), float(original_elbo_weight),
           _ptr(scratch), stream())
    return dict(scalars=scalars, ls=ls, dpred=dpred, dlogvar=dlogvar)


def _vq_dims(z, codebook, idx):
    ops._chk(z, "vq z")
    ops._chk(codebook, "vq codebook")
    n, dim, h, w_ = z.shape
    if not (idx.is_cuda and idx.is_contiguous()) or codebook.shape[1] != dim or idx.dtype != torch.int32 or idx.numel() != n * h * w_:
        raise ValueError(f"vq: z {tuple(z.shape)}, codebook {tuple(codebook.shape)}, idx {idx.dtype} x {idx.numel()} "
                         "(int32, one per latent vector, as ops.vq_nearest writes it)")
    return n, dim, h * w_


def vq_loss_bwd(z, codebook, idx, dzq=None, beta=0.25, legacy=True, w=1.0, dz=None, loss=None, want_dz=True):
    """The codebook loss of VectorQuantizer2 and its gradient w.r.t. the encoder output: z (n,dim,h,w) NCHW, dzq the
    gradient that arrives at the quantised latent (straight-through).  -> (loss[1], dz); loss is not scaled by w."""
    n, dim, hw = _vq_dims(z, codebook, idx)
    for t in (dzq, dz):
        ops._chk(t, "vq_loss_bwd dzq / dz")
        if t is not None and t.shape != z.shape:
            raise ValueError(f"vq_loss_bwd: dzq / dz {tuple(t.shape)} against z {tuple(z.shape)}")
    if want_dz and dz is None:
        dz = torch.empty_like(z)
    loss = _f32(1, device=z.device) if loss is None else loss
    scratch = torch.empty(256, device=z.device, dtype=torch.float64)
    L.call("ldmk_vq_loss_bwd", _ptr(z), _ptr(codebook), _ptr(idx), _ptr(dzq), _ptr(dz), _ptr(loss), n, hw, dim,
           codebook.shape[0], beta, 1 if legacy else 0, w, _ptr(scratch), stream())
    return loss, dz


def vq_codebook_grad(z, codebook, idx, beta=0.25, legacy=True, w=1.0, dE=None, count=None):
    """-> (dE (n_e,dim), count (n_e,) int32): the codebook's gradient of the codebook loss and the hits per code."""
    n, dim, hw = _vq_dims(z, codebook, idx)
    dE = torch.empty_like(codebook) if dE is None else dE
    count = torch.empty(codebook.shape[0], device=z.device, dtype=torch.int32) if count is None else count
    L.call("ldmk_vq_codebook_grad", _ptr(z), _ptr(codebook), _ptr(idx), _ptr(dE), _ptr(count), n, hw, dim,
           codebook.shape[0], beta, 1 if legacy else 0, w, stream())
    return dE, count


def conv1x1_nchw_bwd(x, dy, w, dx=None, dw=None, db=None, accumulate=False, want_dx=True):
    """Backward of ops.conv1x1_nchw: x (n,cin,h,w), dy (n,cout,h,w), w (cout,cin[,1,1]) -> (dx, dw (cout,cin), db)."""
    n, cin, h, w_ = x.shape
    cout = dy.shape[1]
    for t in (x, dy, w, dx, dw, db):
        ops._chk(t, "conv1x1_nchw_bwd")
    if dy.shape != (n, cout, h, w_) or w.numel() != cout * cin or (dx is not None and dx.shape != x.shape):
        raise ValueError(f"conv1x1_nchw_bwd: x {tuple(x.shape)}, dy {tuple(dy.shape)}, w {tuple(w.shape)}")
    if want_dx and dx is None:
        dx = torch.empty_like(x)
    if accumulate and (dw is None or db is None):
        raise ValueError("conv1x1_nchw_bwd: accumulate needs dw and db")
    dw = _f32(cout, cin, device=x.device) if dw is None else dw
    db = _f32(cout, device=x.device) if db is None else db
    scratch = torch.empty(9216, device=x.device, dtype=torch.float64)
    L.call("ldmk_conv1x1_nchw_bwd", _ptr(x), _ptr(dy), _ptr(w), _ptr(dx), _ptr(dw), _ptr(db), n, h * w_, cin, cout,
           1 if accumulate else 0, _ptr(scratch), stream())
    return dx, dw, db


def l1_sum_grad(pred, target, g, dpred=None, total=None):
    """-> (sum|pred - target| [1], dpred = g * sign(pred - target)): the pixel term of the NLL loss, whose gradient scale
    1 / (n exp(logvar)) is real-valued (l1_grad takes an integer denominator and returns the mean)."""
    ops._chk(pred, "l1_sum_grad pred")
    ops._chk(target, "l1_sum_grad target")
    if target.numel() != pred.numel():
        raise ValueError(f"l1_sum_grad: pred {tuple(pred.shape)} against target {tuple(target.shape)}")
    dpred = torch.empty_like(pred) if dpred is None else dpred
    total = _f32(1, device=pred.device) if total is None else total
    scratch = torch.empty(256, device=pred.device, dtype=torch.float64)
    L.call("ldmk_l1_sum_grad", _ptr(pred), _ptr(target), _ptr(dpred), pred.numel(), float(g), _ptr(total), _ptr(scratch), stream())
    return total, dpred


def _kl_dims(moments, what, **same):
    ops._chk(moments, what)
    if moments.dim() != 4 or moments.shape[1] % 2:
        raise ValueError(f"{what}: moments must be (n, 2e, h, w), got {tuple(moments.shape)}")
    n, c2, h, w_ = moments.shape
    for name, t in same.items():
        ops._chk(t, f"{what} {name}")
        if t is not None and tuple(t.shape) != (n, c2 // 2, h, w_):
            raise ValueError(f"{what}: {name} {tuple(t.shape)} against the mean {(n, c2 // 2, h, w_)}")
    return n, c2 // 2, h * w_


def gauss_kl_fwd(moments, noise=None, z=None, kl=None):
    """The KL bottleneck: moments (n,2e,h,w) -> (z (n,e,h,w), kl (n,)).  z = mean + std * noise with the bits of
    ops.gauss_posterior(moments, noise, z=True) (noise None: the mean), kl[b] = 0.5 sum(mean^2 + var - 1 - logvar)."""
    n, e, hw = _kl_dims(moments, "gauss_kl_fwd", noise=noise, z=z)
    z = _f32(n, e, *moments.shape[2:], device=moments.device) if z is None else z
    kl = _f32(n, device=moments.device) if kl is None else kl
    scratch = torch.empty(64 * n, device=moments.device, dtype=torch.float64)
    L.call("ldmk_gauss_kl_fwd", _ptr(moments), _ptr(noise), _ptr(z), _ptr(kl), n, e, hw, _ptr(scratch), stream())
    return z, kl


def gauss_kl_bwd(moments, noise=None, dz=None, w=0.0, dmoments=None):
    """Backward of gauss_kl_fwd for a loss <dz, z> + w * sum_b kl[b] -> dmoments (n,2e,h,w).  dz None: the KL term alone;
    noise None (the mode was decoded): no std term.  The raw log-variance takes gradient on [-30, 20], bounds included."""
    n, e, hw = _kl_dims(moments, "gauss_kl_bwd", noise=noise, dz=dz)
    dmoments = torch.empty_like(moments) if dmoments is None else dmoments
    if dmoments.shape != moments.shape:
        raise ValueError(f"gauss_kl_bwd: dmoments {tuple(dmoments.shape)} against moments {tuple(moments.shape)}")
    ops._chk(dmoments, "gauss_kl_bwd dmoments")
    L.call("ldmk_gauss_kl_bwd", _ptr(moments), _ptr(noise), _ptr(dz), float(w), _ptr(dmoments), n, e, hw, stream())
    return dmoments


# ---- EncoderUNetModel's pooled heads and the classifier's cross-entropy (csrc/classifier.hip): fp32 in both compute modes
def pool_mean(x, n, hw, feat=None, col=0):
    """Mean over the hw rows of an NHWC activation x (n, hw, c) (any shape with n*hw*c elements, c last) into columns
    [col, col + c) of feat (n, ld); feat None: a fresh (n, c)."""
    ops._chk(x, "pool_mean x")
    c = x.shape[-1]
    if x.numel() != n * hw * c:
        raise ValueError(f"pool_mean: x {tuple(x.shape)} is not (n={n}, hw={hw}, c)")
    feat = _f32(n, c, device=x.device) if feat is None else feat
    ops._chk(feat, "pool_mean feat")
    if feat.dim() != 2 or feat.shape[0] != n or col < 0 or col + c > feat.shape[1]:
        raise ValueError(f"pool_mean: columns [{col}, {col + c}) of feat {tuple(feat.shape)} for n={n}")
    L.call("ldmk_pool_mean", _ptr(x), _ptr(feat), n, hw, c, feat.shape[1], col, stream())
    return feat


def pool_mean_bwd(dfeat, n, hw, c, col=0, dx=None, accumulate=False):
    """dx (n, hw, c) (+)= dfeat[:, col:col + c] / hw."""
    ops._chk(dfeat, "pool_mean_bwd dfeat")
    if dfeat.dim() != 2 or dfeat.shape[0] != n or col < 0 or col + c > dfeat.shape[1]:
        raise ValueError(f"pool_mean_bwd: columns [{col}, {col + c}) of dfeat {tuple(dfeat.shape)} for n={n}")
    if dx is None:
        if accumulate:
            raise ValueError("pool_mean_bwd: accumulate needs dx")
        dx = _f32(n, hw, c, device=dfeat.device)
    ops._chk(dx, "pool_mean_bwd dx")
    if dx.numel() != n * hw * c:
        raise ValueError(f"pool_mean_bwd: dx {tuple(dx.shape)} is not (n={n}, hw={hw}, c={c})")
    L.call("ldmk_pool_mean_bwd", _ptr(dfeat), _ptr(dx), n, hw, c, dfeat.shape[1], col, 1 if accumulate else 0, stream())
    return dx


def attnpool_tokens(y, pos_t, n, hw):
    """y (n*hw, c) rows, pos_t (hw + 1, c) -- the transpose of AttentionPool2d.positional_embedding -> X (n*(hw + 1), c)."""
    ops._chk(y, "attnpool_tokens y")
    ops._chk(pos_t, "attnpool_tokens pos_t")
    c = y.shape[-1]
    if y.numel() != n * hw * c or tuple(pos_t.shape) != (hw + 1, c):
        raise ValueError(f"attnpool_tokens: y {tuple(y.shape)}, pos_t {tuple(pos_t.shape)} for n={n}, hw={hw}")
    X = _f32(n * (hw + 1), c, device=y.device)
    L.call("ldmk_attnpool_tokens", _ptr(y), _ptr(pos_t), _ptr(X), n, hw, c, stream())
    return X


def attnpool_tokens_bwd(dX, n, hw, dpos_t=None, accumulate=False, want_dy=True):
    """dX (n*(hw + 1), c) -> (dy (n*hw, c), dpos_t (hw + 1, c) (+)= the sum over the samples, in sample order)."""
    ops._chk(dX, "attnpool_tokens_bwd dX")
    c = dX.shape[-1]
    if dX.numel() != n * (hw + 1) * c:
        raise ValueError(f"attnpool_tokens_bwd: dX {tuple(dX.shape)} for n={n}, hw={hw}")
    if dpos_t is None:
        if accumulate:
            raise ValueError("attnpool_tokens_bwd: accumulate needs dpos_t")
        dpos_t = _f32(hw + 1, c, device=dX.device)
    ops._chk(dpos_t, "attnpool_tokens_bwd dpos_t")
    if dpos_t.numel() != (hw + 1) * c:
        raise ValueError(f"attnpool_tokens_bwd: dpos_t {tuple(dpos_t.shape)} for hw={hw}, c={c}")
    dy = _f32(n * hw, c, device=dX.device) if want_dy else None
    L.call("ldmk_attnpool_tokens_bwd", _ptr(dX), _ptr(dy), _ptr(dpos_t), n, hw, c, 1 if accumulate else 0, stream())
    return dy, dpos_t


def attnpool_fwd(qkv, n, tokens, heads, d_head):
    """Single-query attention of AttentionPool2d: qkv (n*tokens, 3*heads*d_head), columns [q | k | v][head][d] ->
    (out (n, heads*d_head): token 0's attention output, probs (n, heads, tokens) for the backward)."""
    ops._chk(qkv, "attnpool_fwd qkv")
    C_ = heads * d_head
    if qkv.numel() != n * tokens * 3 * C_:
        raise ValueError(f"attnpool_fwd: qkv {tuple(qkv.shape)} for n={n}, tokens={tokens}, heads={heads}, d_head={d_head}")
    out, probs = _f32(n, C_, device=qkv.device), _f32(n, heads, tokens, device=qkv.device)
    L.call("ldmk_attnpool_fwd", _ptr(qkv), _ptr(out), _ptr(probs), n, tokens, heads, int(d_head), stream())
    return out, probs


def attnpool_bwd(qkv, probs, dout, n, tokens, heads, d_head):
    """-> dqkv shaped like qkv, every element written (zeros in the q columns of the tokens past the first)."""
    for name, t in (("qkv", qkv), ("probs", probs), ("dout", dout)):
        ops._chk(t, f"attnpool_bwd {name}")
    C_ = heads * d_head
    if qkv.numel() != n * tokens * 3 * C_ or probs.numel() != n * heads * tokens or dout.numel() != n * C_:
        raise ValueError(f"attnpool_bwd: qkv {tuple(qkv.shape)}, probs {tuple(probs.shape)}, dout {tuple(dout.shape)} for n={n}, "
                         f"tokens={tokens}, heads={heads}, d_head={d_head}")
    dqkv = torch.empty_like(qkv)
    L.call("ldmk_attnpool_bwd", _ptr(qkv), _ptr(probs), _ptr(dout), _ptr(dqkv), n, tokens, heads, int(d_head), stream())
    return dqkv


def cross_entropy(logits, target, scale=None, want_dlogits=True):
    """F.cross_entropy of logits (n, K), 1 <= K <= 1024, against int64 targets (n,): -> (per-sample loss (n,), mean loss [1],
    dlogits = (softmax - onehot) * scale or None).  scale None: 1 / n, the gradient of the mean."""
    ops._chk(logits, "cross_entropy logits")
    if logits.dim() != 2 or not 1 <= logits.shape[1] <= 1024:
        raise ValueError(f"cross_entropy: logits {tuple(logits.shape)}: (n, K) with 1 <= K <= 1024")
    n, K = logits.shape
    if not (target.is_cuda and target.is_contiguous()) or target.dtype != torch.int64 or target.numel() != n:
        raise ValueError(f"cross_entropy: targets {target.dtype} {tuple(target.shape)}: contiguous int64 CUDA, one per row of the logits")
    per, mean = _f32(n, device=logits.device), _f32(1, device=logits.device)
    dl = torch.empty_like(logits) if want_dlogits else None
    L.call("ldmk_cross_entropy", _ptr(logits), _ptr(target), _ptr(per), _ptr(mean), _ptr(dl), float(1.0 / n if scale is None else scale),
           n, K, stream())
    return per, mean, dl


def relu(x, out=None):
    out = torch.empty_like(x) if out is None else out
    L.call("ldmk_relu", _ptr(x), _ptr(out), x.numel(), stream())
    return out


def relu_bwd(x, dy, out=None):
    out = torch.empty_like(x) if out is None else out
    L.call("ldmk_relu_bwd", _ptr(x), _ptr(dy), _ptr(out), x.numel(), stream())
    return out


# ---- LPIPS over VGG16 (csrc/lpips.hip): the kernels around the convolutions; fp32 whatever COMPUTE says
def lpips_conv_in(x, wt, bias, shift, scale, out=None):
    """conv1_1 behind the ScalingLayer: x (n,3,h,w) NCHW, wt (64,3,3,3) OIHW -> relu(conv((x - shift) / scale) + bias), (n,h,w,64) NHWC."""
    for name, t in (("x", x), ("wt", wt), ("bias", bias), ("shift", shift), ("scale", scale), ("out", out)):
        ops._chk(t, f"lpips_conv_in {name}")
    if x.dim() != 4 or x.shape[1] != 3 or wt.numel() != 64 * 27 or bias.numel() != 64 or shift.numel() != 3 or scale.numel() != 3:
        raise ValueError(f"lpips_conv_in: x {tuple(x.shape)}, wt {tuple(wt.shape)}, bias {tuple(bias.shape)}: (n,3,h,w), (64,3,3,3), (64,)")
    n, _, h, w_ = x.shape
    out = _f32(n, h, w_, 64, device=x.device) if out is None else out
    if out.numel() != n * h * w_ * 64:
        raise ValueError(f"lpips_conv_in: out {tuple(out.shape)} for x {tuple(x.shape)}")
    L.call("ldmk_lpips_conv_in", _ptr(x), _ptr(wt), _ptr(bias), _ptr(shift), _ptr(scale), _ptr(out), n, h, w_, stream())
    return out


def lpips_conv_in_bwd(dy, y, wt, scale, dx=None):
    """dy, y (n,h,w,64) NHWC (y: the saved output, the ReLU mask) -> dx (n,3,h,w) NCHW, every element written."""
    for name, t in (("dy", dy), ("y", y), ("wt", wt), ("scale", scale), ("dx", dx)):
        ops._chk(t, f"lpips_conv_in_bwd {name}")
    if dy.dim() != 4 or dy.shape[-1] != 64 or y.shape != dy.shape or wt.numel() != 64 * 27 or scale.numel() != 3:
        raise ValueError(f"lpips_conv_in_bwd: dy {tuple(dy.shape)}, y {tuple(y.shape)}, wt {tuple(wt.shape)}")
    n, h, w_, _ = dy.shape
    dx = _f32(n, 3, h, w_, device=dy.device) if dx is None else dx
    if dx.numel() != n * 3 * h * w_:
        raise ValueError(f"lpips_conv_in_bwd: dx {tuple(dx.shape)} for dy {tuple(dy.shape)}")
    L.call("ldmk_lpips_conv_in_bwd", _ptr(dy), _ptr(y), _ptr(wt), _ptr(scale), _ptr(dx), n, h, w_, stream())
    return dx


def relu_maxpool2(x, relu_out=None, pooled=None):
    """x (n,h,w,c) NHWC pre-activations -> (pooled (n,h//2,w//2,c), relu_out).  relu_out: None (not written), True (a fresh map),
    or a buffer -- x itself is allowed and makes the ReLU in place."""
    ops._chk(x, "relu_maxpool2 x")
    n, h, w_, c = x.shape
    if relu_out is True:
        relu_out = torch.empty_like(x)
    pooled = _f32(n, h // 2, w_ // 2, c, device=x.device) if pooled is None else pooled
    ops._chk(relu_out, "relu_maxpool2 relu_out")
    ops._chk(pooled, "relu_maxpool2 pooled")
    if (relu_out is not None and relu_out.shape != x.shape) or tuple(pooled.shape) != (n, h // 2, w_ // 2, c):
        raise ValueError(f"relu_maxpool2: x {tuple(x.shape)}, pooled {tuple(pooled.shape)}")
    L.call("ldmk_relu_maxpool2", _ptr(x), _ptr(relu_out), _ptr(pooled), n, h, w_, c, stream())
    return pooled, relu_out


def relu_maxpool2_bwd(x, dy, dx=None):
    """x (n,h,w,c): the map the forward read or the post-ReLU map it wrote; dy (n,h//2,w//2,c) -> dx like x, every element written."""
    ops._chk(x, "relu_maxpool2_bwd x")
    ops._chk(dy, "relu_maxpool2_bwd dy")
    n, h, w_, c = x.shape
    if tuple(dy.shape) != (n, h // 2, w_ // 2, c):
        raise ValueError(f"relu_maxpool2_bwd: dy {tuple(dy.shape)} for x {tuple(x.shape)}")
    dx = torch.empty_like(x) if dx is None else dx
    ops._chk(dx, "relu_maxpool2_bwd dx")
    if dx.shape != x.shape:
        raise ValueError(f"relu_maxpool2_bwd: dx {tuple(dx.shape)} for x {tuple(x.shape)}")
    L.call("ldmk_relu_maxpool2_bwd", _ptr(x), _ptr(dy), _ptr(dx), n, h, w_, c, stream())
    return dx


def _lpips_layer_dims(f0, f1, lin, what):
    for name, t in (("f0", f0), ("f1", f1), ("lin", lin)):
        ops._chk(t, f"{what} {name}")
    c = f0.shape[-1]
    n = f0.shape[0]
    if f0.dim() < 3 or f1.shape != f0.shape or lin.numel() != c:
        raise ValueError(f"{what}: taps {tuple(f0.shape)} / {tuple(f1.shape)}, lin {tuple(lin.shape)}: two (n, ..., C) maps and C weights")
    return n, f0[0].numel() // c, c


_LPIPS_PARTIALS = {}     # device -> float64 scratch of ldmk_lpips_layer's per-workgroup partials (64 per sample), stream-ordered reuse


def lpips_layer(f0, f1, lin, res=None, accumulate=False):
    """res[b] (+)= mean over the pixels of sum_c lin_c (u0_c - u1_c)^2, u = f / (|f| + 1e-10): f0, f1 (n,h,w,C) or (n,hw,C) NHWC."""
    n, hw, c = _lpips_layer_dims(f0, f1, lin, "lpips_layer")
    if res is None:
        if accumulate:
            raise ValueError("lpips_layer: accumulate needs res")
        res = _f32(n, device=f0.device)
    ops._chk(res, "lpips_layer res")
    if res.numel() != n:
        raise ValueError(f"lpips_layer: res {tuple(res.shape)} for n={n}")
    scratch = _LPIPS_PARTIALS.get(f0.device)
    if scratch is None or scratch.numel() < 64 * n:
        scratch = _LPIPS_PARTIALS[f0.device] = torch.empty(max(64 * n, 4096), device=f0.device, dtype=torch.float64)
    L.call("ldmk_lpips_layer", _ptr(f0), _ptr(f1), _ptr(lin), _ptr(res), 1 if accumulate else 0, n, hw, c, _ptr(scratch), stream())
    return res


def lpips_layer_bwd(fa, fb, lin, g, df=None, relu_mask=True, accumulate=False):
    """The gradient of lpips_layer with respect to fa, its first tap (the other branch: swap the taps), for g (n,) = dL / dres.
    relu_mask: zero where fa <= 0 (fa is a post-ReLU map; the result is the pre-activation's gradient); accumulate: added to df."""
    n, hw, c = _lpips_layer_dims(fa, fb, lin, "lpips_layer_bwd")
    ops._chk(g, "lpips_layer_bwd g")
    if g.numel() != n:
        raise ValueError(f"lpips_layer_bwd: g {tuple(g.shape)} for n={n}")
    if df is None:
        if accumulate:
            raise ValueError("lpips_layer_bwd: accumulate needs df")
        df = torch.empty_like(fa)
    ops._chk(df, "lpips_layer_bwd df")
    if df.shape != fa.shape:
        raise ValueError(f"lpips_layer_bwd: df {tuple(df.shape)} for fa {tuple(fa.shape)}")
    L.call("ldmk_lpips_layer_bwd", _ptr(fa), _ptr(fb), _ptr(lin), _ptr(g), _ptr(df), 1 if relu_mask else 0, 1 if accumulate else 0,
           n, hw, c, stream())
    return df


def adamw_(p, g, m, v, lr, betas, eps, weight_decay, step):
    L.call("ldmk_adamw", _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, betas[0], betas[1], eps, weight_decay, step, stream())


def ema_(shadow, p, one_minus_decay):
    L.call("ldmk_ema", _ptr(shadow), _ptr(p), p.numel(), one_minus_decay, stream())


def head_permute(src, n, tokens, parts, heads, to_heads, out=None):
    out = torch.empty_like(src) if out is None else out
    L.call("ldmk_head_permute", _ptr(src), _ptr(out), n, tokens, parts, heads, 1 if to_heads else 0, stream())
    return out


def attention_backward(qkv, datt, n, tokens, heads):
    """Gradient of ldmk_attn_self w.r.t. the fused qkv rows: scores re-materialised per head ([n*heads][T][T]) and the
    five products run as batched GEMMs on the matrix cores (attention.py:178-192 backward)."""
    Z, T_, scale = n * heads, tokens, 32 ** -0.5
    dev = qkv.device
    h = head_permute(qkv, n, T_, 3, heads, True).view(3, Z, T_, 32)
    q, k, v = h[0], h[1], h[2]
    do = head_permute(datt, n, T_, 1, heads, True).view(Z, T_, 32)
    p = ops.bmm(q, k, True, alpha=scale)                               # [Z][T][T]
    ops.softmax_rows_(p.view(Z * T_, T_), 1.0)
    dh = torch.empty(3, Z, T_, 32, device=dev)
    _wgrad_batched(p, do, dh[2], Z, T_, T_, 32)                         # dV = P^T dO
    dp = ops.bmm(do, v, True)                                          # dP = dO V^T
    softmax_bwd_rows_(p.view(Z * T_, T_), dp.view(Z * T_, T_), scale)   # dS (scaled)
    ops.bmm(dp, k, False, out=dh[0])                                   # dQ = dS K
    _wgrad_batched(dp, q, dh[1], Z, T_, T_, 32)                         # dK = dS^T Q
    return head_permute(dh, n, T_, 3, heads, False).view(n * T_, 3 * heads * 32)


def _wgrad_batched(a, dy, out, Z, R, Kw, N):
    w = wgrad_args(R, Kw, N, a, dy, out, batch=Z, a_bstride=R * Kw, dy_bstride=R * N, dw_bstride=Kw * N)
    sr, need = wgrad_workspace_elems(w)
    ws = _workspace(a.device, need)
    w.splitr, w.ws, w.ws_elems = sr, ws.data_ptr(), ws.numel()
    wgrad(w)


def attn_self_lse(qkv, n, tokens, heads, d_head=32):
    """Forward attention that also returns the per-row log-sum-exp [n][heads][tokens] (saved for the backward).
    d_head other than 32 (a multiple of 4 in (32, 96]): the fp32 flash kernels of csrc/attention_train.hip, in either compute mode."""
    if d_head != 32:
        out = _f32(n * tokens, heads * d_head, device=qkv.device)
        lse = _f32(n, heads, tokens, device=qkv.device)
        L.call("ldmk_attn_self_lse_d", _ptr(qkv), _ptr(out), _ptr(lse), n, tokens, heads, int(d_head), d_head ** -0.5, stream())
        return out, lse
    out = _f32(n * tokens, heads * 32, device=qkv.device)
    lse = _f32(n, heads, tokens, device=qkv.device)
    # bf16 compute mode: Q K^T and P V on the bf16 matrix cores (fp32 softmax / statistics / storage), like the GEMMs
    name = "ldmk_attn_self_lse_bf16" if COMPUTE == L.COMPUTE_BF16 else "ldmk_attn_self_lse"
    L.call(name, _ptr(qkv), _ptr(out), _ptr(lse), n, tokens, heads, 32 ** -0.5, stream())
    return out, lse


def attn_self_bwd(qkv, out, dout, lse, n, tokens, heads, d_head=32, dqkv=None):
    """d(qkv) of ldmk_attn_self, flash style (probabilities recomputed from lse; any token count).  dqkv: an optional
    contiguous result buffer shaped like qkv; every element of it is written."""
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    elif dqkv.shape != qkv.shape or not dqkv.is_contiguous() or dqkv.dtype != qkv.dtype or dqkv.device != qkv.device:
        raise L.LdmkError(f"attn_self_bwd: dqkv must be a contiguous buffer shaped like qkv ({tuple(dqkv.shape)} vs {tuple(qkv.shape)})")
    dsum = _f32(n * heads * tokens, device=qkv.device)
    if d_head != 32:
        L.call("ldmk_attn_self_bwd_d", _ptr(qkv), _ptr(out), _ptr(dout), _ptr(lse), _ptr(dqkv), _ptr(dsum), n, tokens, heads,
               int(d_head), d_head ** -0.5, stream())
        return dqkv
    name = "ldmk_attn_self_bwd_bf16" if COMPUTE == L.COMPUTE_BF16 else "ldmk_attn_self_bwd"
    L.call(name, _ptr(qkv), _ptr(out), _ptr(dout), _ptr(lse), _ptr(dqkv), _ptr(dsum), n, tokens, heads, 32 ** -0.5, stream())
    return dqkv


def _rows_like(t, out, what):
    """A gradient buffer with exactly t's shape and row stride (the kernels take ONE leading dimension for a tensor and its
    gradient).  torch.empty_like would return a compact tensor for a column slice of a wider buffer."""
    if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise L.LdmkError(f"attn_cross_bwd: {what} must be 2-D rows with unit column stride and a row stride >= its width "
                          f"(shape {tuple(t.shape)}, strides {tuple(t.stride())})")
    if out is None:
        return torch.empty_strided(t.shape, t.stride(), device=t.device, dtype=t.dtype)
    if out.shape != t.shape or out.stride() != t.stride() or out.dtype != t.dtype or out.device != t.device:
        raise L.LdmkError(f"attn_cross_bwd: d{what} must have the shape and strides of {what} "
                          f"({tuple(out.shape)} / {tuple(out.stride())} vs {tuple(t.shape)} / {tuple(t.stride())})")
    return out


def attn_cross_bwd(q, k, v, dout, n, tokens, ctx_len, heads, dq=None, dk=None, dv=None, d_head=32):
    """Gradients of ldmk_attn_cross: q [n*tokens][C], k / v [n*ctx_len][C], dout [n*tokens][C] -> (dq, dk, dv).
    Row strides may exceed C (column slices of wider buffers); every gradient has the row stride of its input, and k and v
    must share one.  d_head other than 32: ldmk_attn_cross_bwd_d (40, 64, 80)."""
    if k.stride(0) != v.stride(0):
        raise L.LdmkError(f"attn_cross_bwd: k and v must share one row stride ({k.stride(0)} vs {v.stride(0)})")
    if dout.dim() != 2 or dout.stride(1) != 1 or dout.stride(0) < dout.shape[1]:
        raise L.LdmkError(f"attn_cross_bwd: dout must be 2-D rows with unit column stride (strides {tuple(dout.stride())})")
    dq, dk, dv = _rows_like(q, dq, "q"), _rows_like(k, dk, "k"), _rows_like(v, dv, "v")
    scratch = _f32(2 * n * tokens * heads * ctx_len, device=q.device)
    if d_head != 32:
        L.call("ldmk_attn_cross_bwd_d", _ptr(q), q.stride(0), _ptr(k), _ptr(v), k.stride(0), _ptr(dout), dout.stride(0), _ptr(dq),
               _ptr(dk), _ptr(dv), _ptr(scratch), n, tokens, ctx_len, heads, int(d_head), d_head ** -0.5, stream())
        return dq, dk, dv
    L.call("ldmk_attn_cross_bwd", _ptr(q), q.stride(0), _ptr(k), _ptr(v), k.stride(0), _ptr(dout), dout.stride(0), _ptr(dq),
           _ptr(dk), _ptr(dv), _ptr(scratch), n, tokens, ctx_len, heads, 32 ** -0.5, stream())
    return dq, dk, dv
