"""GPU: the KL first stage -- the moment head and the posterior kernel at the smallest shapes that can go wrong, against
float64 from the same fp32 operands; the call surface against the reference's recorded outputs (tests/golden/g20_kl.npz and
g20_kl_patch.npz, made by tools/make_golden_kl.py from the real reference classes); std-rescaling, one training step, graph
replay, and a VQ model afterwards to show that the base the two autoencoders share changed nothing."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, rnd

pytestmark = pytest.mark.gpu

SCALE = 0.18215
T = lambda a: torch.from_numpy(np.asarray(a))
SPLIT = dict(ks=(32, 32), stride=(16, 16), vqf=4, patch_distributed_vq=True, tie_braker=False, clip_min_weight=0.01,
             clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
PATCH = dict(f4=(48, 64, SPLIT), f8=(12, 16, dict(SPLIT, ks=(8, 8), stride=(4, 4), vqf=8)))
TRAIN_UNET = dict(model_channels=64, channel_mult=[1, 2], num_res_blocks=1, attention_resolutions=[2, 1])     # g9's


def close(a, b, rtol=1e-4, atol=1e-4):
    torch.testing.assert_close(a.float().cpu(), torch.as_tensor(np.asarray(b)).float(), rtol=rtol, atol=atol)


@pytest.fixture(scope="module")
def ops():
    from dsml_thesis_amd import lib, ops as ops_
    lib.load()
    return ops_


@pytest.fixture(scope="module")
def g20():
    return golden("g20_kl.npz")


def _model(tag, unet=None, gain=0.25, **kw):
    from dsml_thesis_amd import synth
    kl = dict(f4=synth.KL_F4, f8=synth.KL_F8_SMALL)[tag]
    e = kl["embed_dim"]
    return synth.make_kl_model(gain=gain, unet=dict(synth.FR_UNET, in_channels=e, out_channels=e, **(unet or {})), kl=kl, **kw)


@pytest.fixture(scope="module")
def models():
    """f4: the shipped UNet at gain 0.25 (g5's sampling model) under a KL-f4 first stage; f8: g9's small UNet, 4 channels."""
    return dict(f4=_model("f4"), f8=_model("f8", TRAIN_UNET))


# ------------------------------------------------------------------------------------------ ldmk_conv3x3_moments
HEAD_CASES = [(2, 64, 6, 6, 17, 18, True),          # ragged second tile in both axes
              (1, 36, 8, 6, 5, 7, False),           # cin not a multiple of 32, one partial tile, no-norm path, c2e != c2z
              (2, 512, 8, 8, 8, 8, True),           # the KL-f8 head
              (1, 128, 2, 4, 1, 1, True),           # a single pixel, all halo
              (1, 160, 4, 2, 32, 32, True)]


@pytest.mark.parametrize("n,cin,c2z,c2e,h,w,norm", HEAD_CASES, ids=lambda v: str(v))
def test_moment_head_against_float64(ops, n, cin, c2z, c2e, h, w, norm):
    """float64 conv2d(silu(group_norm(x))) then the float64 1x1, from the same fp32 operands, at test_conv3x3_out_tiles' inputs and
    its 1e-4 / 1e-4 (the project's bound for this tile and this silu_f)."""
    x = rnd(170, n, cin, h, w) * 1.4
    w3, b3 = rnd(171, c2z, cin, 3, 3) / np.sqrt(9 * cin), rnd(172, c2z)
    w1, b1 = rnd(175, c2e, c2z, 1, 1) / np.sqrt(c2z), rnd(176, c2e)
    xs = x.permute(0, 2, 3, 1).contiguous().cuda()
    coef, ref_in = None, x.double()
    if norm:
        gamma, beta = 1 + 0.1 * rnd(173, cin), 0.1 * rnd(174, cin)
        coef = ops.gn_coef(xs, None, n, h * w, gamma.cuda(), beta.cuda(), 1e-5)
        ref_in = F.silu(F.group_norm(x.double(), 32, gamma.double(), beta.double(), 1e-5))
    want = F.conv2d(F.conv2d(ref_in, w3.double(), b3.double(), padding=1), w1.double(), b1.double())
    w3p, w1d = ops.pack_conv3x3_narrow(w3.cuda()), w1.reshape(c2e, c2z).contiguous().cuda()
    got = ops.conv3x3_moments(xs, coef, w3p, b3.cuda(), w1d, b1.cuda())
    assert got.shape == (n, c2e, h, w)
    print(f"moment head {(n, cin, c2z, c2e, h, w, norm)}: max |err| {(got.double().cpu() - want).abs().max().item():.3e}, "
          f"max |ref| {want.abs().max().item():.3e}")
    torch.testing.assert_close(got.double().cpu(), want, rtol=1e-4, atol=1e-4)
    assert torch.equal(ops.conv3x3_moments(xs, coef, w3p, b3.cuda(), w1d, b1.cuda()), got), "one fixed summation order"
    if c2z <= 4:         # identity 1x1, zero 1x1 bias: the boundary conv the project already has, on the same operands
        eye = torch.eye(c2z, device="cuda")
        ident = ops.conv3x3_moments(xs, coef, w3p, b3.cuda(), eye, torch.zeros(c2z, device="cuda"))
        torch.testing.assert_close(ident, ops.conv3x3_out(xs, coef, w3p, b3.cuda(), c2z), rtol=2e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------ ldmk_gauss_posterior
def _logvar_grid(numel):
    """A grid over [-40, 30] that holds -30, 20 and the fp32 neighbours on both sides of each: both clamp branches run (the
    two out-of-range neighbours come first, so that even the two elements of the smallest case take one branch each)."""
    lo, hi, inf = np.float32(-30.0), np.float32(20.0), np.float32(np.inf)
    edge = [np.nextafter(lo, -inf), np.nextafter(hi, inf), lo, hi, np.nextafter(lo, inf), np.nextafter(hi, -inf)]
    grid = np.concatenate([np.array(edge, np.float32), np.linspace(-40.0, 30.0, 4099).astype(np.float32)])
    return torch.from_numpy(np.resize(grid, numel).astype(np.float32))


@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (32, 32)], ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("c2", [2, 6, 8])
def test_gauss_posterior_against_float64(ops, c2, hw):
    """n = 2.  A sample's plane of e*h*w floats decides the kernel: 1x1 and 5x7 take the scalar one (5x7 with 2e = 8 has a
    plane of 140 floats and takes the 16-byte one), 32x32 the 16-byte one."""
    n, e, (h, w) = 2, c2 // 2, hw
    mean = rnd(300 + c2, n, e, h, w) * 2.0
    lv = _logvar_grid(n * e * h * w).reshape(n, e, h, w)
    lv = lv.flatten()[torch.from_numpy(np.random.RandomState(5).permutation(lv.numel()))].reshape(n, e, h, w) if h * w > 1 else lv
    moments = torch.cat([mean, lv], 1).contiguous().cuda()
    noise = rnd(310 + c2, n, e, h, w).cuda()
    scale = float(np.float32(SCALE))                             # the fp32 operand the kernel is handed
    o = ops.gauss_posterior(moments, noise=noise, scale=scale, logvar=True, std=True, var=True, z=True)
    clamped = lv.clamp(-30.0, 20.0)
    assert torch.equal(o["logvar"].cpu(), clamped), "clamped logvar is bit-exact"
    assert (lv < -30.0).any() and (lv > 20.0).any(), "both clamp branches run"
    assert lv.numel() < 6 or ((lv == -30.0).any() and (lv == 20.0).any() and ((lv > -30.0) & (lv < 20.0)).any())
    # std / var: the bound is measured here, on torch.exp (the reference implementation) against float64 on the same
    # arguments; the kernel gets twice that, with a floor of 2^-23
    rel = lambda got, arg: ((got.double().cpu() - torch.exp(arg.double())).abs() / torch.exp(arg.double())).max().item()
    half = 0.5 * clamped
    t_std, t_var = rel(torch.exp(half.cuda()), half), rel(torch.exp(clamped.cuda()), clamped)
    k_std, k_var = rel(o["std"], half), rel(o["var"], clamped)
    print(f"gauss posterior c2={c2} {h}x{w}: rel err std kernel {k_std:.3e} / torch.exp {t_std:.3e}; "
          f"var kernel {k_var:.3e} / torch.exp {t_var:.3e}")
    assert k_std <= max(2 * t_std, 2.0 ** -23) and k_var <= max(2 * t_var, 2.0 ** -23)
    # z from the kernel's own fp32 mean, std and noise: one rounding each for the product, the sum and the scale
    m64, s64, n64 = mean.double(), o["std"].double().cpu(), noise.double().cpu()
    err = (o["z"].double().cpu() - scale * (m64 + s64 * n64)).abs()
    bound = 3 * 2.0 ** -24 * scale * (m64.abs() + (s64 * n64).abs())
    assert (err <= bound).all(), (err / bound.clamp_min(1e-300)).max().item()
    # subsets of the outputs, and the draws without noise
    only = ops.gauss_posterior(moments, std=True)
    assert set(only) == {"std"} and torch.equal(only["std"], o["std"])
    zm = ops.gauss_posterior(moments, scale=scale, z=True)["z"].double().cpu()
    assert ((zm - scale * m64).abs() <= 2.0 ** -24 * scale * m64.abs()).all(), "noise null: z = scale * mean to one rounding"
    assert torch.equal(ops.gauss_posterior(moments, scale=1.0, z=True)["z"].cpu(), mean), "scale 1: z is the mean, bitwise"
    # an unaligned base pointer (a view one float in) takes the scalar kernel and agrees bit for bit
    flat = torch.empty(moments.numel() + 1, device="cuda")
    flat[1:].copy_(moments.flatten())
    shifted = flat[1:].view_as(moments)
    o2 = ops.gauss_posterior(shifted, noise=noise, scale=scale, logvar=True, std=True, var=True, z=True)
    assert all(torch.equal(o2[k], o[k]) for k in o)


# ------------------------------------------------------------------------------------------ against the reference (g20)
@pytest.mark.parametrize("tag,res", [("f4", 128), ("f8", 64)])
def test_encode_sample_decode_against_the_reference(models, g20, tag, res):
    from dsml_thesis_amd.distributions import DiagonalGaussianDistribution
    m = models[tag]
    x = rnd(201, 2, 3, res, res).cuda()
    post = m.encode_first_stage(x)
    assert isinstance(post, DiagonalGaussianDistribution)
    ref = T(g20[f"{tag}_moments"])
    print(f"[{tag}] moments: max |diff| vs the reference {(post.parameters.cpu() - ref).abs().max().item():.3e}")
    close(post.parameters, ref, 1e-4, 1e-4)
    noise = T(g20[f"{tag}_noise"])
    z = m.get_first_stage_encoding(post, noise=noise.cuda())
    e = ref.shape[1] // 2
    std = torch.exp(0.5 * ref[:, e:].clamp(-30.0, 20.0))
    tol = SCALE * 1e-4 * (1 + (0.5 * std * noise.abs()).max().item())          # the moments bound through mean + exp(logvar/2) noise
    print(f"[{tag}] z: max |diff| vs the reference {(z.cpu() - T(g20[f'{tag}_z'])).abs().max().item():.3e}, tolerance {tol:.3e}")
    close(z, g20[f"{tag}_z"], tol, tol)
    dec = m.decode_first_stage(T(g20[f"{tag}_z"]).cuda())
    print(f"[{tag}] decoded: max |diff| vs the reference {(dec.cpu() - T(g20[f'{tag}_decoded'])).abs().max().item():.3e}")
    close(dec, g20[f"{tag}_decoded"], 1e-4, 1e-4)
    fs = m.first_stage_model
    out, post2 = fs(x, sample_posterior=False)
    assert torch.equal(out, fs.decode(fs.encode(x).mode())) and torch.equal(post2.parameters, post.parameters)
    torch.manual_seed(3)
    out_s, _ = fs(x)                                              # sample_posterior=True: decode(mean + std * randn)
    torch.manual_seed(3)
    nz = torch.randn(post.mean.shape, device="cuda")
    assert torch.equal(out_s, fs.decode(post.sample(noise=nz)))
    with pytest.raises(TypeError):
        fs.decode(z, force_not_quantize=True)                     # the reference signature has no such argument


@pytest.mark.parametrize("tag", ["f4", "f8"])
def test_patch_wise_decode(models, tag):
    from dsml_thesis_amd import ops
    from dsml_thesis_amd.patches import patch_geometry
    m = models[tag]
    h, w, split = PATCH[tag]
    ks, st, uf = split["ks"][0], split["stride"][0], split["vqf"]
    e = m.first_stage_model.embed_dim
    z = rnd(204, 1, e, h, w).cuda()
    want = golden("g20_kl_patch.npz")[f"{tag}_patch_decoded"]
    m.split_input_params = dict(split)
    try:
        dec = m.decode_first_stage(z, force_not_quantize=True)     # (the flag is dropped for a first stage that is not VQ)
        with pytest.raises(NotImplementedError, match="AutoencoderKL"):
            m.encode_first_stage(rnd(205, 1, 3, uf * ks, uf * ks).cuda())
    finally:
        del m.split_input_params
    print(f"[{tag}] patch-wise decode: max |diff| vs the reference {(dec.cpu() - T(want)).abs().max().item():.3e}")
    close(dec, want, 1e-4, 1e-4)
    ly, lx, weight, norm = patch_geometry((h, w), (ks, ks), (st, st), uf=uf, params=split, device="cuda")
    crops = ops.patch_unfold(1. / SCALE * z, ks, ks, st, st)
    outs = [m.first_stage_model.decode(crops[l:l + 1]) for l in range(ly * lx)]
    o = torch.stack(outs, dim=-1) * weight.view(1, 1, uf * ks, uf * ks, ly * lx)
    fold = torch.nn.Fold(output_size=(uf * h, uf * w), kernel_size=(uf * ks, uf * ks), dilation=1, padding=0, stride=(uf * st, uf * st))
    ref = fold(o.reshape(1, -1, ly * lx)) / norm.view(1, 1, uf * h, uf * w)
    close(dec, ref.cpu(), 2e-4, 2e-4)


def test_std_rescaling_on_the_first_batch(g20, monkeypatch):
    m = _model("f8", TRAIN_UNET, scale_factor=1.0, scale_by_std=True)
    assert isinstance(m.scale_factor, torch.Tensor) and "scale_factor" in dict(m.named_buffers())
    batch = dict(image=rnd(201, 2, 3, 64, 64).permute(0, 2, 3, 1).contiguous())
    noise = T(g20["f8_std_noise"]).cuda()
    real_randn = torch.randn
    shape_of = lambda a: tuple(a[0]) if isinstance(a[0], (tuple, list, torch.Size)) else tuple(a)
    monkeypatch.setattr(torch, "randn", lambda *a, **k: noise if shape_of(a) == tuple(noise.shape) else real_randn(*a, **k))
    m.restarted_from_ckpt = True
    m.on_train_batch_start(batch, 0, 0)
    assert float(m.scale_factor) == 1.0, "a run restarted from a checkpoint keeps its scale_factor"
    m.restarted_from_ckpt = False
    m.on_train_batch_start(batch, 1, 0)
    assert float(m.scale_factor) == 1.0, "only the very first batch"
    m.on_train_batch_start(batch, 0, 0)
    want = float(g20["f8_std_scale_factor"])
    print(f"std-rescaling: scale_factor {float(m.scale_factor):.7f}, reference {want:.7f}")
    assert abs(float(m.scale_factor) - want) <= 1e-4 * want
    assert "scale_factor" in m.state_dict() and m.scale_factor.is_cuda
    first = m.scale_factor.clone()
    m.on_train_batch_start(batch, 0, 0)
    assert torch.equal(m.scale_factor, first), "a second call changes nothing"
    m2 = _model("f8", TRAIN_UNET, scale_factor=0.5, scale_by_std=True)
    with pytest.raises(AssertionError, match="std-rescaling"):
        m2.on_train_batch_start(batch, 0, 0)


def test_training_step_from_an_image_batch(models):
    m = models["f8"].train()
    try:
        batch = dict(image=rnd(210, 2, 3, 128, 128).permute(0, 2, 3, 1).contiguous(), class_label=torch.tensor([1, 5]).cuda())
        torch.manual_seed(21)
        z, _ = m.get_input(batch, "image")
        torch.manual_seed(21)
        nz = torch.randn(z.shape, device="cuda")
        post = m.encode_first_stage(batch["image"].permute(0, 3, 1, 2).contiguous().cuda())
        want = SCALE * (post.mean.double() + post.std.double() * nz.double())
        bound = 3 * 2.0 ** -24 * SCALE * (post.mean.double().abs() + (post.std.double() * nz.double()).abs())
        assert z.shape == (2, 4, 16, 16) and ((z.double() - want).abs() <= bound).all()
        loss = m.training_step(batch, 0)
        assert torch.isfinite(loss).all() and float(loss) > 0
    finally:
        m.eval()


def test_ddim_sample_then_decode_graph_equals_eager(models):
    from dsml_thesis_amd.ddim import DDIMSampler
    m = models["f4"]
    lab = torch.tensor((1, 6), device="cuda")[:, None]
    c = m.cond_stage_model.embedding(lab)
    xT = rnd(51, 2, 3, 32, 32).cuda()
    kw = dict(S=4, batch_size=2, shape=[3, 32, 32], conditioning=c, eta=0.0, x_T=xT, verbose=False)
    out, _ = DDIMSampler(m).sample(**kw)
    out_g, _ = DDIMSampler(m).sample(use_graph=True, **kw)
    assert torch.equal(out, out_g)
    close(out, golden("g5_sampling_fr.npz")["sample_S4"], 1.5e-4, 1.5e-4)      # the sampler does not touch the first stage
    img, img_g = m.decode_first_stage(out), m.decode_first_stage(out_g)
    assert img.shape == (2, 3, 128, 128) and torch.isfinite(img).all() and torch.equal(img, img_g)
    with pytest.raises(NotImplementedError, match="no `quantize`"):
        DDIMSampler(m).sample(quantize_x0=True, **kw)


def test_a_vq_model_afterwards_is_unchanged(models):
    """The base the two autoencoders share emits VQModelInterface's programs as before: g6's `encoded` and code indices."""
    from helpers import make_fr_model
    g = golden("g6_vqgan.npz")
    m = make_fr_model()
    close(m.encode_first_stage(torch.tanh(rnd(64, 1, 3, 128, 128)).cuda()), g["encoded"], 1e-4, 1e-4)
    _, idx = m.first_stage_model.decode(rnd(61, 1, 3, 32, 32).cuda(), return_indices=True)
    assert np.array_equal(idx.cpu().numpy(), g["vq_idx"].reshape(-1))
