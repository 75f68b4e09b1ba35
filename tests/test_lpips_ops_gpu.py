"""GPU: the kernels of csrc/lpips.hip through their wrappers in train_ops, each against the float64 restatement tests/lpips_ref.py
from the same fp32 operands.

Bounds come from the number format, not from what the kernels give.  With u = 2^-24 and K the number of roundings on the longest
path to an output (the in-lane fused multiply-adds, six butterfly levels of a 64-lane sum, the divisions, square roots and
products around them), an output that is a sum of terms t_i carries at most K u sum|t_i|, the magnitudes taken from float64:
  conv_in        K = 32 (27 fused multiply-adds, the subtraction and division of the ScalingLayer, the bias): 32 u (|b| + sum |w| |s|)
  conv_in_bwd    K = 24 (9 taps in-lane, 6 levels, the division): 24 u sum |dy| |w| / scale over the unmasked taps
  lpips_layer    K = 32 (8 in-lane + 6 levels for each of two norms and the sum, sqrt, reciprocal, products):
                 32 u mean_pixels sum_c w_c (|u0_c| + |u1_c|)^2
  lpips_layer_bwd  K = 32: 32 u (r A_k + |f_k| r^2 / n sum_c A_c |f_c|),  A_c = 2 w_c (|ua_c| + |ub_c|) |g| / hw  -- |ua| + |ub| and not
                 |ua - ub|, because the rounding of either term does not shrink when they cancel; accumulate adds u |result|
The pooling kernels move values and are compared exactly, on small integers so that ties are real.
Every output lies inside a frame of sentinel floats that must stay intact, gradients are prefilled with NaN, every kernel runs
twice for identical bits, and bad arguments return LDMK_EINVAL with the output untouched."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R
from conftest import rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _grad_mode_on():
    """some modules of the suite switch autograd off process-wide when they are imported; these tests differentiate"""
    with torch.enable_grad():
        yield

U = 2.0 ** -24
SENT = -12345.5
PAD = 1024                      # floats of frame on either side (a multiple of 4: the framed tensor stays 16-byte aligned)
SHIFT, SCALE = torch.tensor([-.030, -.088, -.188]), torch.tensor([.458, .448, .450])


@pytest.fixture(scope="module")
def T():
    from dsml_thesis_amd import lib, train_ops
    lib.load()
    return train_ops


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_error():
    """A sticky HIP error ends the session: nothing more is launched on a device that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error during this test, nothing more is launched: {e}", returncode=3)


class Framed:
    """A contiguous fp32 CUDA tensor inside a frame of SENT; `fill` is what the interior holds before the kernel writes it."""

    def __init__(self, shape, fill=float("nan"), offset=0):
        numel = int(np.prod(shape))
        self.flat = torch.full((numel + 2 * PAD + offset,), SENT, device="cuda")
        self.t = self.flat[PAD + offset:PAD + offset + numel].view(shape)
        self.t.fill_(fill)
        self.lo, self.hi = PAD + offset, PAD + offset + numel

    def intact(self):
        return bool((self.flat[:self.lo] == SENT).all() and (self.flat[self.hi:] == SENT).all())


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _within(what, got, ref, bound):
    err = (got.detach().double().cpu() - ref).abs()
    over = (err - bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, max bound {bound.max().item():.3e}, max |ref| {ref.abs().max().item():.3e}, "
          f"worst err/bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert torch.isfinite(got).all() and over <= 0, f"{what}: {over:.3e} over its bound"


# ------------------------------------------------------------------------------------------ conv_in
@pytest.mark.parametrize("h,w", [(5, 7), (16, 16), (260, 128)])
def test_conv_in_and_its_backward(T, h, w):
    """260 x 128 x 2 = 66560 pixels against 4 x 16384 per pass of the grid: the grid-stride loops of both kernels lap."""
    n = 2
    x = rnd(2800 + h, n, 3, h, w)
    wt = rnd(2801, 64, 3, 3, 3) * float(np.sqrt(2.0 / 27))
    bias = rnd(2802, 64) * 0.5
    out = Framed((n, h, w, 64))
    args = [t.cuda().contiguous() for t in (x, wt, bias, SHIFT, SCALE)]
    T.lpips_conv_in(*args, out=out.t)
    ref = R.conv_in(x, wt, bias, SHIFT, SCALE)
    s_abs = ((x.double() - SHIFT.double().view(1, 3, 1, 1)) / SCALE.double().view(1, 3, 1, 1)).abs()
    bound = 32 * U * (F.conv2d(s_abs, wt.double().abs(), padding=1) + bias.double().abs().view(1, -1, 1, 1))
    _within(f"conv_in {h}x{w}", nchw(out.t), ref, bound)
    y = out.t.clone()
    frac = (y > 0).float().mean().item()
    assert 0.2 < frac < 0.8, f"the ReLU mask has both kinds ({frac:.2f} positive)"
    assert out.intact()
    T.lpips_conv_in(*args, out=out.t)
    assert torch.equal(out.t, y), "two runs, identical bits"
    # the padding is of the SCALED tensor: a constant image equal to the shift scales to zero everywhere, border included
    flat = SHIFT.view(1, 3, 1, 1).expand(1, 3, h, w).contiguous().cuda()
    o2 = T.lpips_conv_in(flat, *args[1:])
    assert torch.equal(o2, torch.relu(args[2]).view(1, 1, 1, 64).expand(1, h, w, 64)), "shift not folded into the bias"
    # backward, with the kernel's own output as the mask
    dy = rnd(2803 + h, n, 64, h, w)
    dx = Framed((n, 3, h, w))
    T.lpips_conv_in_bwd(nhwc(dy).cuda(), y, args[1], args[4], dx=dx.t)
    ymask = nchw(y).cpu()
    refb = R.conv_in_bwd(dy, ymask, wt, SCALE)
    gabs = torch.where(ymask > 0, dy.double().abs(), torch.zeros((), dtype=torch.float64))
    boundb = 24 * U * F.conv_transpose2d(gabs, wt.double().abs(), padding=1) / SCALE.double().view(1, 3, 1, 1)
    _within(f"conv_in_bwd {h}x{w}", dx.t, refb, boundb)
    assert dx.intact()
    first = dx.t.clone()
    dx.t.fill_(float("nan"))
    T.lpips_conv_in_bwd(nhwc(dy).cuda(), y, args[1], args[4], dx=dx.t)
    assert torch.equal(dx.t, first), "two runs, identical bits"


# ------------------------------------------------------------------------------------------ relu + maxpool
def _ints(seed, *shape, lo=-2, hi=2):
    return torch.from_numpy(np.random.RandomState(seed).randint(lo, hi + 1, size=shape).astype(np.float32))


@pytest.mark.parametrize("h,w,offset", [(6, 3, 0), (7, 5, 0), (2, 2, 0), (7, 5, 1)], ids=lambda v: str(v))
def test_relu_maxpool2_and_its_backward_exactly(T, h, w, offset):
    """Integers in [-2, 2]: ties in most windows, windows with nothing positive.  offset 1: pointers one float off a 16-byte boundary,
    the scalar form."""
    n, c = 2, 64
    x = _ints(2810 + h, n, c, h, w)
    x[0, :, 0:2, 0:2] = torch.tensor([[2., 2.], [2., 1.]])                 # a positive tie: the first in row-major order
    x[1, :, 0:2, 0:2] = torch.tensor([[-1., 0.], [-2., 0.]])               # nothing positive
    xg = Framed((n, h, w, c), offset=offset)
    xg.t.copy_(nhwc(x))
    assert xg.t.data_ptr() % 16 == 4 * offset
    pooled, relu = Framed((n, h // 2, w // 2, c), offset=offset), Framed((n, h, w, c), offset=offset)
    T.relu_maxpool2(xg.t, relu_out=relu.t, pooled=pooled.t)
    pref, rref = R.relu_maxpool2(x)
    assert torch.equal(nchw(pooled.t).cpu().double(), pref) and torch.equal(nchw(relu.t).cpu().double(), rref)
    assert pooled.intact() and relu.intact() and xg.intact() and torch.equal(xg.t.cpu(), nhwc(x)), "x is only read"
    p_only = Framed((n, h // 2, w // 2, c), offset=offset)
    T.relu_maxpool2(xg.t, pooled=p_only.t)
    assert torch.equal(p_only.t, pooled.t), "without relu_out: the same pooled map"
    inplace = Framed((n, h, w, c), offset=offset)
    inplace.t.copy_(xg.t)
    T.relu_maxpool2(inplace.t, relu_out=inplace.t, pooled=p_only.t)
    assert torch.equal(inplace.t, relu.t) and torch.equal(p_only.t, pooled.t) and inplace.intact(), "relu_out = x: in place"
    # backward
    dy = _ints(2811 + h, n, c, h // 2, w // 2, lo=1, hi=9)
    dref = R.relu_maxpool2_bwd(x, dy)
    leaf = x.double().clone().requires_grad_(True)
    auto, = torch.autograd.grad((F.max_pool2d(F.relu(leaf), 2, 2) * dy.double()).sum(), leaf)
    assert torch.equal(dref, auto), "the restated scan is torch's own routing"
    for what, src in (("pre-activation", xg.t), ("post-ReLU", relu.t)):
        dx = Framed((n, h, w, c), offset=offset)
        T.relu_maxpool2_bwd(src, nhwc(dy).cuda(), dx=dx.t)
        got = nchw(dx.t).cpu().double()
        assert not torch.isnan(got).any(), f"{what}: every element of dx is written"
        assert torch.equal(got, dref), what
        assert dx.intact()
        assert (got[0, :, 0, 0] == dy[0, :, 0, 0].double()).all() and (got[0, :, 0:2, 0:2].sum(dim=(1, 2)) == dy[0, :, 0, 0].double()).all(), \
            "a positive tie routes to the first maximum alone"
        assert (got[1, :, 0:2, 0:2] == 0).all(), "a window with nothing positive takes no gradient"
        if h % 2:
            assert (got[:, :, h - 1, :] == 0).all(), "the dropped row"
        if w % 2:
            assert (got[:, :, :, w - 1] == 0).all(), "the dropped column"
        again = Framed((n, h, w, c), offset=offset)
        T.relu_maxpool2_bwd(src, nhwc(dy).cuda(), dx=again.t)
        assert torch.equal(again.t, dx.t), "two runs, identical bits"


def test_relu_maxpool2_grid_stride_laps(T):
    """2 x 65 x 65 windows x 64 float4 channel groups = 540800 threads' worth against 2048 x 256 per pass: both loops lap."""
    n, c, h, w = 2, 256, 130, 130
    x = _ints(2815, n, c, h, w)
    xg = nhwc(x).cuda()
    pooled, relu = T.relu_maxpool2(xg, relu_out=True)
    pref, rref = R.relu_maxpool2(x)
    assert torch.equal(nchw(pooled).cpu().double(), pref) and torch.equal(nchw(relu).cpu().double(), rref)
    dy = _ints(2816, n, c, h // 2, w // 2, lo=1, hi=9)
    dx = Framed((n, h, w, c))
    T.relu_maxpool2_bwd(relu, nhwc(dy).cuda(), dx=dx.t)
    assert torch.equal(nchw(dx.t).cpu().double(), R.relu_maxpool2_bwd(x, dy)) and dx.intact()


# ------------------------------------------------------------------------------------------ the LPIPS layer
# C = 64 / 512 at 1, 3 and 35 pixels; C = 256 at 300 pixels: 75 workgroups' worth against the forward's cap of 64 per sample, its
# loop laps; C = 128 at 4100 pixels: 8200 against 4 x 2048 per pass of the backward's grid, that loop laps -- so every width of the
# template (1, 2, 4, 8 floats per lane) runs
LAYER_CASES = [(64, 1), (64, 3), (64, 35), (512, 1), (512, 3), (512, 35), (256, 300), (128, 4100)]


def _taps(c, hw, n=2):
    """post-ReLU-like taps (n, C, hw, 1) with an all-zero vector in fa (sample 1, last pixel) and in fb (sample 0, first pixel)"""
    fa, fb = torch.relu(rnd(2820 + c + hw, n, c, hw, 1)), torch.relu(rnd(2821 + c + hw, n, c, hw, 1) + 0.3)
    fa[1, :, hw - 1] = 0
    fb[0, :, 0] = 0
    lin = torch.from_numpy(np.random.RandomState(2822 + c).uniform(0, 1, c).astype(np.float32))
    return fa, fb, lin, torch.tensor([0.7, -1.3])


@pytest.mark.parametrize("c,hw", LAYER_CASES, ids=lambda v: str(v))
def test_lpips_layer_forward(T, c, hw):
    fa, fb, lin, _ = _taps(c, hw)
    a, b, w = nhwc(fa).cuda(), nhwc(fb).cuda(), lin.cuda()
    res = Framed((2,))
    T.lpips_layer(a, b, w, res=res.t)
    ref = R.layer(fa, fb, lin)
    ua, ub = R.normalize(fa.double())[0].abs(), R.normalize(fb.double())[0].abs()
    bound = 32 * U * (lin.double().view(1, -1, 1, 1) * (ua + ub) ** 2).sum(dim=1).mean(dim=(1, 2))
    _within(f"lpips_layer C={c} hw={hw}", res.t, ref, bound)
    first = res.t.clone()
    T.lpips_layer(a, b, w, res=res.t, accumulate=True)
    assert torch.equal(res.t, first + first), "accumulate: one fp32 add of the same value"
    T.lpips_layer(a, b, w, res=res.t)
    assert torch.equal(res.t, first) and res.intact(), "two runs, identical bits"


@pytest.mark.parametrize("c,hw", LAYER_CASES, ids=lambda v: str(v))
def test_lpips_layer_backward_both_branches(T, c, hw):
    fa, fb, lin, g = _taps(c, hw)
    w, gg = lin.cuda(), g.cuda()
    dev = dict(a=nhwc(fa).cuda(), b=nhwc(fb).cuda())
    cpu = dict(a=fa, b=fb)
    for first, second in (("a", "b"), ("b", "a")):                              # the branch differentiated is the FIRST tap
        f1, f2 = cpu[first].double(), cpu[second].double()
        ref = R.layer_bwd(f1, f2, lin, g)
        u1, n1 = R.normalize(f1)
        u2, _ = R.normalize(f2)
        A = 2.0 * lin.double().view(1, -1, 1, 1) * (u1.abs() + u2.abs()) * g.double().abs().view(-1, 1, 1, 1) / hw
        r = 1.0 / (n1 + R.EPS)
        safe = torch.where(n1 > 0, n1, torch.ones_like(n1))
        bound = 32 * U * (r * A + f1.abs() * torch.where(n1 > 0, r * r / safe, torch.zeros_like(n1)) * (A * f1.abs()).sum(dim=1, keepdim=True))
        zero = (n1 == 0).expand_as(f1)
        assert zero.any(), "one pixel of this branch is an all-zero vector"
        for mask in (False, True):
            want = torch.where(f1 > 0, ref, torch.zeros_like(ref)) if mask else ref
            df = Framed(tuple(dev[first].shape))
            T.lpips_layer_bwd(dev[first], dev[second], w, gg, df=df.t, relu_mask=mask)
            got = nchw(df.t.view(2, hw, 1, c))
            _within(f"lpips_layer_bwd d/d{first} C={c} hw={hw} mask={mask}", got, want, bound)
            assert df.intact()
            if mask:
                assert (got.cpu()[f1 <= 0] == 0).all(), "an exact zero where the tap is not positive"
            else:
                zv = got.cpu().double()[zero]
                assert torch.isfinite(zv).all() and (zv != 0).any(), "the all-zero vector takes the finite r * a"
            base = rnd(2830 + hw, *dev[first].shape).cuda()
            acc = Framed(tuple(dev[first].shape))
            acc.t.copy_(base)
            T.lpips_layer_bwd(dev[first], dev[second], w, gg, df=acc.t, relu_mask=mask, accumulate=True)
            assert torch.equal(acc.t, base + df.t), "accumulate: one fp32 add of the same value onto what df held"
            again = Framed(tuple(dev[first].shape))
            T.lpips_layer_bwd(dev[first], dev[second], w, gg, df=again.t, relu_mask=mask)
            assert torch.equal(again.t, df.t) and acc.intact(), "two runs, identical bits"


# ------------------------------------------------------------------------------------------ argument validation
def test_bad_arguments_return_an_error_and_launch_nothing(T):
    from dsml_thesis_amd import lib as L
    lib = L.load()
    out = torch.full((4096,), SENT, device="cuda")
    src = torch.ones(4096, device="cuda")
    scr = torch.zeros(256, device="cuda", dtype=torch.float64)
    p, o, s, st = src.data_ptr(), out.data_ptr(), scr.data_ptr(), torch.cuda.current_stream().cuda_stream
    bad = [
        ("ldmk_lpips_layer", (p, p, p, o, 0, 2, 4, 96, s, st)),                # C not in the set
        ("ldmk_lpips_layer", (p, p, p, o, 0, 0, 4, 64, s, st)),                # n = 0
        ("ldmk_lpips_layer", (p, None, p, o, 0, 2, 4, 64, s, st)),             # null tap
        ("ldmk_lpips_layer", (p, p, p, o, 0, 2, 4, 64, None, st)),             # null scratch
        ("ldmk_lpips_layer", (p + 4, p, p, o, 0, 2, 4, 64, s, st)),            # a tap off the 16-byte boundary
        ("ldmk_lpips_layer_bwd", (p, p, p, p, o, 1, 0, 2, 4, 32, st)),
        ("ldmk_lpips_layer_bwd", (p, p, p, p, None, 1, 0, 2, 4, 64, st)),
        ("ldmk_lpips_layer_bwd", (p, p, p, p, o, 1, 0, 0, 4, 64, st)),
        ("ldmk_lpips_conv_in", (p, p, p, p, p, o, 0, 4, 4, st)),
        ("ldmk_lpips_conv_in", (p, p, None, p, p, o, 1, 4, 4, st)),
        ("ldmk_lpips_conv_in_bwd", (p, p, p, p, None, 1, 4, 4, st)),
        ("ldmk_lpips_conv_in_bwd", (p, p, p, p, o, 1, 0, 4, st)),
        ("ldmk_relu_maxpool2", (p, None, o, 0, 4, 4, 64, st)),
        ("ldmk_relu_maxpool2", (p, None, None, 1, 4, 4, 64, st)),
        ("ldmk_relu_maxpool2", (p, None, o, 1, 1, 4, 64, st)),                 # no room for a window
        ("ldmk_relu_maxpool2_bwd", (p, p, o, 0, 4, 4, 64, st)),
        ("ldmk_relu_maxpool2_bwd", (None, p, o, 1, 4, 4, 64, st)),
        ("ldmk_relu_maxpool2_bwd", (p, p, p, 1, 4, 4, 64, st)),                # dx = x
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, f"{name}{args} is LDMK_EINVAL"
        assert name.encode() in lib.ldmk_last_error()
    torch.cuda.synchronize()
    assert (out == SENT).all() and (src == 1).all(), "nothing was launched"
    with pytest.raises(L.LdmkError, match="64, 128, 256, 512"):
        T.lpips_layer(torch.ones(1, 2, 96, device="cuda"), torch.ones(1, 2, 96, device="cuda"), torch.ones(96, device="cuda"))
