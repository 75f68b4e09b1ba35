"""GPU: the kernels of KL first-stage training (csrc/kl_train.hip), each against float64 from the same fp32 operands.

Bounds.  Reductions (kl, the pixel sum): the torch fp32 formulation on the GPU is measured against the same float64
reference and the kernel gets twice that, with a floor of 2^-23 of max |ref| -- DESIGN §17's rule, the one
test_vq_train_ops_gpu.py uses.  Both figures are printed.  Elementwise outputs have bounds from the number format, stated
where they are used.  Every moments tensor with room for them carries raw log-variances of exactly -30 and 20 (inside the
clamp: they take gradient), the next float outside each bound (no gradient) and +-40."""
import math

import numpy as np
import pytest
import torch

from conftest import rnd

pytestmark = pytest.mark.gpu

W = 0.75                      # exact in fp32: the kernel and the float64 reference see the same operand
LO_OUT = float(np.nextafter(np.float32(-30.0), np.float32(-np.inf)))
HI_OUT = float(np.nextafter(np.float32(20.0), np.float32(np.inf)))
SPECIAL = [-30.0, 20.0, LO_OUT, HI_OUT, 40.0, -40.0]          # [takes gradient] * 2, [takes none] * 4
# (n, e, hw, misaligned): one element; the scalar path (plane % 4 != 0); the 16-byte path; 16-byte-able planes behind pointers
# offset by one float (scalar form); a plane of 131072 floats -- 128 workgroups' worth against the forward's cap of 64 per
# sample, so its grid-stride loop laps
PLANES = [(1, 1, 1, False), (2, 3, 5, False), (2, 4, 64, False), (2, 3, 64, True), (3, 4, 32768, False)]


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


def _offset(t):
    """the same values behind a pointer one float past a 16-byte boundary"""
    flat = torch.empty(t.numel() + 1, device=t.device)
    assert flat.data_ptr() % 16 == 0
    flat[1:].copy_(t.flatten())
    return flat[1:].view(t.shape)


def _operands(n, e, hw, misaligned):
    mom = rnd(800 + hw, n, 2 * e, hw, 1)
    mom[:, e:] *= 1.5
    flat = mom[:, e:].clone().reshape(-1)         # the special values, spread evenly over the samples' log-variances
    k = min(len(SPECIAL), flat.numel())
    pos = torch.arange(k) * (flat.numel() // k)
    flat[pos] = torch.tensor(SPECIAL[:k])
    mom[:, e:] = flat.view(n, e, hw, 1)
    noise, dz = rnd(801 + hw, n, e, hw, 1), rnd(802 + hw, n, e, hw, 1)
    ts = [t.cuda().contiguous() for t in (mom, noise, dz)]
    if misaligned:
        ts = [_offset(t) for t in ts]
        assert all(t.data_ptr() % 16 == 4 for t in ts)
    return ts + [pos, k]


@pytest.mark.parametrize("n,e,hw,misaligned", PLANES, ids=lambda v: str(v))
def test_gauss_kl_forward_against_float64(T, n, e, hw, misaligned):
    from dsml_thesis_amd import ops
    mom, noise, dz, pos, k = _operands(n, e, hw, misaligned)
    raw = mom[:, e:].reshape(-1).cpu()
    assert k == 1 or all((raw == v).any() for v in SPECIAL), "every special log-variance is present"
    z, kl = T.gauss_kl_fwd(mom, noise)
    aligned = mom.clone()
    assert torch.equal(z, ops.gauss_posterior(aligned, noise=noise.clone(), z=True)["z"]), "the posterior kernel's draw, bit for bit"
    zm, klm = T.gauss_kl_fwd(mom, None)
    assert torch.equal(zm, mom[:, :e]) and torch.equal(zm, ops.gauss_posterior(aligned, z=True)["z"]), "noise = null: the mean"
    assert torch.equal(klm, kl), "kl does not depend on the noise"
    z2, kl2 = T.gauss_kl_fwd(mom, noise)
    assert torch.equal(kl, kl2) and torch.equal(z, z2), "two calls, identical bits"
    assert kl.shape == (n,) and z.shape == (n, e, hw, 1)
    m64, l64 = mom[:, :e].double().cpu(), mom[:, e:].double().cpu().clamp(-30.0, 20.0)
    ref = 0.5 * (m64 ** 2 + torch.exp(l64) - 1.0 - l64).sum(dim=(1, 2, 3))
    l32 = mom[:, e:].clamp(-30.0, 20.0)
    kl32 = 0.5 * (mom[:, :e] ** 2 + torch.exp(l32) - 1.0 - l32).sum(dim=(1, 2, 3))
    _reduction_ok("kl", kl, kl32, ref)
    if misaligned:                                   # the 16-byte form on the same values: another order, the same bound
        _, kla = T.gauss_kl_fwd(aligned, noise.clone())
        _reduction_ok("kl, 16-byte form", kla, kl32, ref)


@pytest.mark.parametrize("n,e,hw,misaligned", PLANES, ids=lambda v: str(v))
def test_gauss_kl_backward_against_float64(T, n, e, hw, misaligned):
    """d mean = fma(w, mean, dz): one rounding, |err| <= 2^-24 (|dz| + |w mean|).  d raw = 0.5 fma(fl(dz noise), std, fl(w fl(var - 1)))
    with std, var from expf (1 ulp): the three roundings on the std term and the three on the var term are each 2^-24 or 2^-23 of
    their term, under 2^-21 (|dz noise std| + |w| (var + 1)) together; the factor 0.5 is exact."""
    mom, noise, dz, pos, k = _operands(n, e, hw, misaligned)
    m64, raw64 = mom[:, :e].double().cpu(), mom[:, e:].double().cpu()
    inside = (raw64 >= -30.0) & (raw64 <= 20.0)
    flat_in = inside.reshape(-1)[pos]
    assert flat_in.tolist() == [True, True, False, False, False, False][:k], "bounds take gradient, the next floats outside do not"
    std, var = torch.exp(0.5 * raw64), torch.exp(raw64)
    n64, g64 = noise.double().cpu(), dz.double().cpu()
    for form, (nz, g) in dict(full=(noise, dz), no_dz=(noise, None), no_noise=(None, dz), neither=(None, None)).items():
        out = T.gauss_kl_bwd(mom, nz, g, W)
        assert out.shape == mom.shape
        gg = g64 if g is not None else torch.zeros_like(g64)
        st = gg * n64 * std if (nz is not None and g is not None) else torch.zeros_like(g64)
        dm_ref = gg + W * m64
        dl_ref = torch.where(inside, 0.5 * (st + W * (var - 1.0)), torch.zeros_like(var))
        dm, dl = out[:, :e].double().cpu(), out[:, e:].double().cpu()
        b_m = 2.0 ** -24 * (gg.abs() + (W * m64).abs())
        b_l = torch.where(inside, 2.0 ** -21 * (st.abs() + W * (var + 1.0)), torch.zeros_like(var))
        assert ((dm - dm_ref).abs() <= b_m).all(), f"{form}: d mean, worst {((dm - dm_ref).abs() - b_m).max():.3e} over"
        assert ((dl - dl_ref).abs() <= b_l).all(), f"{form}: d log-variance, worst {((dl - dl_ref).abs() - b_l).max():.3e} over"
        assert (dl[~inside] == 0).all(), f"{form}: outside [-30, 20] the gradient is an exact zero"
        if k > 1:
            assert (dl.reshape(-1)[pos[:2]] != 0).all(), f"{form}: at -30 and at 20 the gradient passes"
        assert torch.equal(out, T.gauss_kl_bwd(mom, nz, g, W)), "two calls, identical bits"
    # w = 0 and no noise: d mean is dz itself, and the log-variance takes nothing
    out = T.gauss_kl_bwd(mom, None, dz, 0.0)
    assert torch.equal(out[:, :e], dz) and (out[:, e:] == 0).all()


@pytest.mark.parametrize("n,misaligned", [(1, False), (37, False), (4096, True), (4 * 256 * 256 * 2, False), (256 * 256 * 3 + 5, False)],
                         ids=lambda v: str(v))
def test_l1_sum_grad_with_ties_and_a_nan(T, n, misaligned):
    """dpred = g sign(pred - target) exactly (one fp32 constant or its negation or a zero); the sum adds |fl(pred - target)|:
    the subtraction's rounding, 2^-24 of each term and all of one sign, plus the final rounding bound it by 2^-23 of the
    sum.  n = 524288 is 512 workgroups' worth of 16-byte accesses against the cap of 256: the loop laps; 196613 is the scalar
    form doing the same."""
    g = 1.0 / (2 * math.exp(-0.7))                   # 1 / (n exp(logvar)): no integer denominator
    pred, target = rnd(820, n), rnd(821, n)
    target[::7] = pred[::7]
    p, t = pred.cuda(), target.cuda()
    if misaligned:
        p, t = _offset(p), _offset(t)
    d = pred.double() - target.double()
    total, dp = T.l1_sum_grad(p, t, g)
    ref = d.abs().sum()
    err = abs(total.double().cpu().item() - ref.item())
    print(f"l1 sum: kernel {err:.3e} / bound {2.0 ** -23 * ref.item():.3e}")
    assert err <= 2.0 ** -23 * ref.item()
    g32 = torch.tensor(g, dtype=torch.float32)
    assert torch.equal(dp.cpu(), torch.sign(pred - target) * g32), "dpred = g sign; sign(0) = 0"
    assert (dp.cpu()[::7] == 0).all()
    total2, dp2 = T.l1_sum_grad(p, t, g)
    assert torch.equal(total, total2) and torch.equal(dp, dp2), "two calls, identical bits"
    # a NaN stays a NaN, in the gradient and in the sum
    p2 = p.clone()
    p2[n // 2] = float("nan")
    total3, dp3 = T.l1_sum_grad(p2, t.clone(), g)
    assert torch.isnan(dp3[n // 2]) and torch.isnan(dp3).sum() == 1 and torch.isnan(total3).all()


def test_l1_grad_keeps_its_bits_next_to_the_new_entry_point(T):
    """ldmk_l1_grad is untouched: its dpred is sign / denom rounded once and its loss the mean, as before; the new entry point
    called with g = fl(1 / denom) writes the same gradient bits."""
    n, denom = 256 * 256 * 3 + 5, 256 * 256 * 2 + 3
    pred, target = rnd(720, n), rnd(721, n)
    target[::7] = pred[::7]
    d = pred.double() - target.double()
    for dn in (denom, 0):
        loss, dp = T.l1_grad(pred.cuda(), target.cuda(), denom=dn)
        dd = dn or n
        assert torch.equal(dp.cpu(), (torch.sign(d) / dd).float())
        assert abs(loss.double().cpu().item() - d.abs().sum().item() / dd) <= 2.0 ** -23 * d.abs().sum().item() / dd
        total, dp2 = T.l1_sum_grad(pred.cuda(), target.cuda(), float(np.float32(1.0 / dd)))
        assert torch.equal(dp2, dp)
        assert abs(total.item() / dd - loss.item()) <= 2.0 ** -22 * loss.item()
