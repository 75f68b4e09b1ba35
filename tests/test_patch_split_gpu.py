"""GPU: the patch-wise mode (`model.split_input_params = {...}`, ddpm.py:565-652,716-753,828-859,904-986) -- the two kernels
against torch, the call surface against the reference's recorded outputs (tests/golden/g19_split.npz, made by
tools/make_golden_split.py from the real reference classes), and crops-as-batch against crops one by one on this repo's own
kernels."""
import contextlib
import math
import types

import numpy as np
import pytest
import torch

from conftest import golden, rnd
from helpers import make_fr_model

pytestmark = pytest.mark.gpu

SPLIT = dict(ks=(32, 32), stride=(16, 16), vqf=4, patch_distributed_vq=True, tie_braker=False, clip_min_weight=0.01,
             clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
H, W_ = 48, 64                                  # Ly = 2, Lx = 3: a transposed patch index cannot pass


def close(a, b, tol):
    torch.testing.assert_close(a.float().cpu(), torch.as_tensor(np.asarray(b)).float(), rtol=tol, atol=tol)


@contextlib.contextmanager
def split(m, **over):
    m.split_input_params = dict(SPLIT, **over)
    try:
        yield m
    finally:
        del m.split_input_params


@pytest.fixture(scope="module")
def fr():
    return make_fr_model(gain=0.25)


@pytest.fixture(scope="module")
def g19():
    return golden("g19_split.npz")


def _cond(m, labels=(1, 6)):
    lab = torch.tensor(labels, device="cuda")[:, None]
    return m.cond_stage_model.embedding(lab), m.cond_stage_model.uncond_embedding(torch.zeros_like(lab))


# ------------------------------------------------------------------------------------------ the two kernels
#          n  c  H   W   kh kw  sh sw
SHAPES = [(2, 3, 12, 20, 8, 12, 4, 8),          # kh != kw, sh != sw, 16-byte path
          (3, 4, 7, 9, 3, 5, 2, 2),             # odd sizes, scalar path, stride does not divide ks, cover counts 1-6
          (1, 3, 8, 8, 8, 8, 8, 8),             # one patch
          (2, 3, 16, 24, 8, 8, 8, 8),           # no overlap, Ly != Lx
          (2, 3, 16, 16, 8, 8, 4, 4)]           # (the tie-breaker case below uses this one too)


def torch_unfold(x, kh, kw, sh, sw):
    n, c = x.shape[:2]
    u = torch.nn.Unfold(kernel_size=(kh, kw), dilation=1, padding=0, stride=(sh, sw))(x)       # (n, c*kh*kw, L)
    L_ = u.shape[-1]
    return u.view(n, c, kh, kw, L_).permute(4, 0, 1, 2, 3).reshape(L_ * n, c, kh, kw).contiguous()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unfold_equals_torch_unfold_bit_for_bit(shape):
    from dsml_thesis_amd import ops
    n, c, h, w, kh, kw, sh, sw = shape
    x = rnd(700 + h, n, c, h, w).cuda()
    got = ops.patch_unfold(x, kh, kw, sh, sw)
    want = torch_unfold(x, kh, kw, sh, sw)
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(ops.patch_unfold(x, kh, kw, sh, sw), got)


@pytest.mark.parametrize("shape,tie", [(s, False) for s in SHAPES] + [(SHAPES[4], True)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("tie" if v else "plain"))
def test_fold_against_float64(shape, tie):
    """out = fold(patches * weight) / norm in float64 from the same fp32 operands.  Per output element the kernel rounds K products
    and K - 1 sums and one quotient, K <= ceil(kh/sh) ceil(kw/sw) patches covering it, and the weights are positive with
    sum(weight) = norm: |error| <= (K + 2) 2^-24 max|patches|."""
    from dsml_thesis_amd import ops
    from dsml_thesis_amd.patches import patch_geometry
    n, c, h, w, kh, kw, sh, sw = shape
    ly, lx, weight, norm = patch_geometry((h, w), (kh, kw), (sh, sw), params=dict(SPLIT, tie_braker=tie), device="cuda")
    L_ = ly * lx
    assert (ly, lx) == ((h - kh) // sh + 1, (w - kw) // sw + 1)
    patches = rnd(800 + h + w, L_ * n, c, kh, kw).cuda()
    got = ops.patch_fold(patches, weight, norm, n, sh, sw)
    o = patches.double().view(L_, n, c, kh, kw).permute(1, 2, 3, 4, 0) * weight.double().view(1, 1, kh, kw, L_)
    fold = torch.nn.Fold(output_size=(h, w), kernel_size=(kh, kw), dilation=1, padding=0, stride=(sh, sw))
    want = fold(o.reshape(n, c * kh * kw, L_)) / norm.double().view(1, 1, h, w)
    K = math.ceil(kh / sh) * math.ceil(kw / sw)
    bound = (K + 2) * 2.0 ** -24 * patches.abs().max().item()
    err = (got.double() - want).abs().max().item()
    print(f"fold {shape} tie={tie}: max |err| {err:.3e}, bound {bound:.3e} (K = {K})")
    assert got.shape == (n, c, h, w) and err <= bound, (err, bound)
    assert torch.equal(ops.patch_fold(patches, weight, norm, n, sh, sw), got), "the fold has one fixed summation order"


def test_fold_of_unfold_is_the_identity_up_to_rounding():
    """Cropping an image and blending the crops back returns it: every pixel is a convex combination of copies of itself."""
    from dsml_thesis_amd import ops
    from dsml_thesis_amd.patches import patch_geometry
    x = rnd(820, 2, 3, H, W_).cuda()
    ly, lx, weight, norm = patch_geometry((H, W_), (32, 32), (16, 16), params=SPLIT, device="cuda")
    back = ops.patch_fold(ops.patch_unfold(x, 32, 32, 16, 16), weight, norm, 2, 16, 16)
    assert (back - x).abs().max().item() <= 6 * 2.0 ** -24 * x.abs().max().item()            # K = 4 products and sums, one quotient


# ------------------------------------------------------------------------------------------ against the reference (g19)
def test_apply_model_against_the_reference(fr, g19):
    c, _ = _cond(fr)
    x, t = rnd(191, 2, 3, H, W_).cuda(), torch.tensor([137, 842], device="cuda")
    with split(fr):
        eps = fr.apply_model(x, t, c)
        d = (eps.cpu() - torch.from_numpy(g19["eps"])).abs().max().item()
        print(f"patch-wise apply_model: max |diff| vs the reference {d:.3e}")
        # the single-evaluation bound: the fold is a convex combination of crop outputs and cannot widen a per-crop error
        close(eps, g19["eps"], 3e-5)
        assert torch.equal(fr.apply_model(x, t, [c]), eps)
        with pytest.raises(NotImplementedError, match="return_ids"):
            fr.apply_model(x, t, c, return_ids=True)


def test_first_stage_against_the_reference(fr, g19):
    z, img = rnd(193, 1, 3, H, W_).cuda(), rnd(194, 1, 3, 4 * H, 4 * W_).cuda()
    with split(fr):
        dec = fr.decode_first_stage(z, force_not_quantize=True)
        assert dec.shape == (1, 3, 4 * H, 4 * W_)
        print(f"patch-wise decode: max |diff| vs the reference {(dec.cpu() - torch.from_numpy(g19['decoded_noquant'])).abs().max().item():.3e}")
        close(dec, g19["decoded_noquant"], 1e-4)
        enc = fr.encode_first_stage(img)
        assert tuple(fr.split_input_params["original_image_size"]) == (4 * H, 4 * W_)
        print(f"patch-wise encode: max |diff| vs the reference {(enc.cpu() - torch.from_numpy(g19['encoded'])).abs().max().item():.3e}")
        close(enc, g19["encoded"], 1e-4)
    with split(fr, patch_distributed_vq=False):                    # the plain path (ddpm.py:754-758, :861-862)
        assert torch.equal(fr.decode_first_stage(z[:, :, :32, :32]), fr.first_stage_model.decode(z[:, :, :32, :32]))
        assert torch.equal(fr.encode_first_stage(img[:, :, :128, :128]), fr.first_stage_model.encode(img[:, :, :128, :128]))


@pytest.mark.parametrize("cfg", [False, True], ids=["cfg1", "cfg3"])
def test_ddim_sample_against_the_reference_and_graph_replay(fr, g19, cfg):
    from dsml_thesis_amd.ddim import DDIMSampler
    c, uc = _cond(fr)
    xT = rnd(192, 2, 3, H, W_).cuda()
    kw = dict(S=4, batch_size=2, shape=[3, H, W_], conditioning=c, eta=0.0, x_T=xT, verbose=False)
    if cfg:
        kw.update(unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    ref = g19["sample_S4_cfg" if cfg else "sample_S4"]
    with split(fr):
        s = DDIMSampler(fr)
        out, _ = s.sample(**kw)
        print(f"patch-wise DDIM S=4 cfg={cfg}: max |diff| vs the reference {(out.cpu() - torch.from_numpy(ref)).abs().max().item():.3e} "
              f"(|x| up to {np.abs(ref).max():.1f})")
        close(out, ref, 1.5e-4)                                    # the g5 trajectory bound: 4 chained evaluations
        out_g, _ = s.sample(use_graph=True, **kw)
        assert torch.equal(out, out_g), "hipGraph replay must be bitwise identical to eager launches"
        out_g2, _ = s.sample(use_graph=True, **kw)
        assert torch.equal(out, out_g2), "a cached graph replays from a clean state"


# ------------------------------------------------------------------------------------------ crops as batch == crops one by one
def _blend(outs, weight, norm, h, w, ks, stride):
    """The reference's own stitching (ddpm.py:981-986) in torch: Fold(weight * stack(outs)) / norm."""
    L_ = len(outs)
    o = torch.stack(outs, dim=-1) * weight.view(1, 1, ks, ks, L_)
    fold = torch.nn.Fold(output_size=(h, w), kernel_size=(ks, ks), dilation=1, padding=0, stride=(stride, stride))
    return fold(o.reshape(o.shape[0], -1, L_)) / norm.view(1, 1, h, w)


def test_apply_model_equals_the_crops_one_by_one(fr):
    from dsml_thesis_amd import ops
    from dsml_thesis_amd.patches import patch_geometry
    c, _ = _cond(fr)
    x, t = rnd(195, 2, 3, H, W_).cuda(), torch.tensor([20, 940], device="cuda")
    ly, lx, weight, norm = patch_geometry((H, W_), (32, 32), (16, 16), params=SPLIT, device="cuda")
    crops = ops.patch_unfold(x, 32, 32, 16, 16).view(ly * lx, 2, 3, 32, 32)
    ref = _blend([fr.model(crops[l], t, c_crossattn=[c]) for l in range(ly * lx)], weight, norm, H, W_, 32, 16)
    with split(fr):
        eps = fr.apply_model(x, t, c)
    print(f"crops as batch vs one by one: max |diff| {(eps - ref).abs().max().item():.3e}")
    close(eps, ref.cpu(), 6e-5)                                    # two evaluations, each within 3e-5 of the exact result


def test_quantised_decode_equals_the_crops_one_by_one(fr):
    from dsml_thesis_amd import ops
    from dsml_thesis_amd.patches import patch_geometry
    z = rnd(196, 1, 3, H, W_).cuda()
    ly, lx, weight, norm = patch_geometry((H, W_), (32, 32), (16, 16), uf=4, params=SPLIT, device="cuda")
    crops = ops.patch_unfold(z, 32, 32, 16, 16)
    _, idx_batch = fr.first_stage_model.decode(crops, return_indices=True)
    one = [fr.first_stage_model.decode(crops[l:l + 1], return_indices=True) for l in range(ly * lx)]
    assert torch.equal(idx_batch.reshape(ly * lx, -1), torch.stack([i.reshape(-1) for _, i in one])), "every crop is quantised on its own"
    ref = _blend([im for im, _ in one], weight, norm, 4 * H, 4 * W_, 128, 64)
    with split(fr):
        dec = fr.decode_first_stage(z)
    print(f"quantised patch-wise decode vs one by one: max |diff| {(dec - ref).abs().max().item():.3e}")
    close(dec, ref.cpu(), 2e-4)


def test_concat_conditioning_is_cropped_with_the_latent():
    """conditioning_key 'concat' with an image-like cond_stage_key: the reference unfolds the conditioning tensor too (ddpm.py:919-929)."""
    from dsml_thesis_amd import ops, synth
    from dsml_thesis_amd.ddpm import LatentDiffusion
    from dsml_thesis_amd.patches import patch_geometry
    cfg = synth.uncond_config(dict(synth.UNCOND_UNET, image_size=32, in_channels=6, out_channels=3), synth.VQ_F4)
    cfg.update(conditioning_key="concat", cond_stage_config="__is_first_stage__", cond_stage_key="image", channels=3, image_size=32)
    m = LatentDiffusion(**cfg)
    synth.load_recipe(m.model.diffusion_model, gain=0.25)
    m = m.cuda().eval()
    x, cc, t = rnd(197, 2, 3, H, W_).cuda(), rnd(198, 2, 3, H, W_).cuda(), torch.tensor([5, 700], device="cuda")
    ly, lx, weight, norm = patch_geometry((H, W_), (32, 32), (16, 16), params=SPLIT, device="cuda")
    xs = ops.patch_unfold(x, 32, 32, 16, 16).view(ly * lx, 2, 3, 32, 32)
    cs = ops.patch_unfold(cc, 32, 32, 16, 16).view(ly * lx, 2, 3, 32, 32)
    ref = _blend([m.model(xs[l], t, c_concat=[cs[l]]) for l in range(ly * lx)], weight, norm, H, W_, 32, 16)
    with split(m):
        eps = m.apply_model(x, t, cc)
        other = m.apply_model(x, t, cc.flip(3))
    close(eps, ref.cpu(), 6e-5)
    assert not torch.equal(eps, other)
    m.cond_stage_key = "class_label"                               # not image-like: every crop would get the full-size tensor
    with split(m), pytest.raises(ValueError, match="full-size"):
        m.apply_model(x, t, cc)


# ------------------------------------------------------------------------------------------ other behaviour
def test_p_sample_loop_is_patch_wise_and_graph_equals_eager(fr):
    c, _ = _cond(fr)
    xT = rnd(199, 2, 3, H, W_).cuda()
    nz = [rnd(900 + k, 2, 3, H, W_).cuda() for k in range(3)]
    plain = fr.p_sample_loop(c, (2, 3, H, W_), x_T=xT, timesteps=3, noise=nz, verbose=False)
    with split(fr):
        eager = fr.p_sample_loop(c, (2, 3, H, W_), x_T=xT, timesteps=3, noise=nz, verbose=False)
        graph = fr.p_sample_loop(c, (2, 3, H, W_), x_T=xT, timesteps=3, noise=nz, verbose=False, use_graph=True)
        # the loop is the chain of single patch-wise steps (p_sample -> apply_model -> the same kernels)
        img = xT
        for k, i in enumerate(reversed(range(3))):
            img = fr.p_sample(img, c, torch.full((2,), i, device="cuda", dtype=torch.long), noise=nz[k])
        # noise drawn inside the step: this is the run that captures unfold -> program -> fold -> update into a hipGraph
        torch.manual_seed(3)
        drawn = fr.p_sample_loop(c, (2, 3, H, W_), x_T=xT, timesteps=3, verbose=False, use_graph=True)
        torch.manual_seed(3)
        drawn2 = fr.p_sample_loop(c, (2, 3, H, W_), x_T=xT, timesteps=3, verbose=False, use_graph=True)
    assert torch.isfinite(eager).all() and torch.equal(eager, graph)
    assert torch.equal(eager, img)
    assert torch.isfinite(drawn).all() and torch.equal(drawn, drawn2), "a cached graph replays the same seeded run"
    assert not torch.equal(eager, plain), "split_input_params is no longer ignored by the sampling loop"
    again = fr.p_sample_loop(c, (2, 3, H, W_), x_T=xT, timesteps=3, noise=nz, verbose=False)
    assert torch.equal(again, plain), "a plain run after a patch-wise one is unchanged"


def test_without_the_attribute_nothing_changes(fr):
    """A patch-wise run first -- at 32x32 with ks 32 it is ONE crop per item, i.e. the very launch program of the plain run --
    then the plain paths against their own fixtures: g5 `sample_S4` (this model) and g4 `fr_eps` (gain 1)."""
    from dsml_thesis_amd.ddim import DDIMSampler
    c, _ = _cond(fr)
    xT = rnd(51, 2, 3, 32, 32).cuda()
    kw = dict(S=4, batch_size=2, shape=[3, 32, 32], conditioning=c, eta=0.0, x_T=xT, verbose=False)
    with split(fr):
        patched, _ = DDIMSampler(fr).sample(use_graph=True, **kw)
    assert not hasattr(fr, "split_input_params")
    out, _ = DDIMSampler(fr).sample(**kw)
    close(out, golden("g5_sampling_fr.npz")["sample_S4"], 1.5e-4)
    out_g, _ = DDIMSampler(fr).sample(use_graph=True, **kw)
    assert torch.equal(out, out_g)
    close(patched, out.cpu(), 1.5e-4)                              # (one crop: the blend is x * w / w)
    m1 = make_fr_model(gain=1.0)
    x, t, ctx = rnd(41, 2, 3, 32, 32).cuda(), torch.tensor([3, 981], device="cuda"), rnd(42, 2, 1, 512).cuda()
    with split(m1):
        m1.apply_model(x, t, ctx)
    close(m1.apply_model(x, t, ctx), golden("g4_unet_fr.npz")["fr_eps"], 3e-5)


def test_what_the_reference_refuses_is_refused(fr):
    from dsml_thesis_amd.ddim import DDIMSampler
    from dsml_thesis_amd.ddpm import LatentDiffusion2Cond
    c, _ = _cond(fr)
    x, t = rnd(191, 2, 3, H, W_).cuda(), torch.tensor([137, 842], device="cuda")
    with split(fr):
        with pytest.raises(NotImplementedError, match="more than one conditioning"):       # hybrid: assert len(cond) == 1
            fr.apply_model(x, t, {"c_crossattn": [c], "c_concat": [x]})
        with pytest.raises(NotImplementedError, match="more than one conditioning"):
            DDIMSampler(fr).sample(S=4, batch_size=2, shape=[3, H, W_], conditioning={"c_crossattn": [c], "c_concat": [x]},
                                   x_T=x, verbose=False)
        with pytest.raises(ValueError, match="do not cover"):                                # 50 rows: the last two would be 0/0
            fr.apply_model(rnd(1, 2, 3, 50, 64).cuda(), t, c)
    two = types.SimpleNamespace(split_input_params=dict(SPLIT))
    with pytest.raises(NotImplementedError, match="split_input_params"):                     # ddpm2cond.py:937-938
        LatentDiffusion2Cond.apply_model(two, x, t, c, x)
