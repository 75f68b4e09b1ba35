"""CPU: the KL-regularised and identity first stages -- factory rows, parameter trees against the reference's recorded key
list (tests/golden/g20_kl.npz, made by tools/make_golden_kl.py from the real reference classes), what is refused, the
oracle as the CPU yardstick for the fixture, the host-side `kl` / `nll` / `normal_kl`, and the argument validation of the
two new entry points (it precedes any launch, so it needs no GPU)."""
import numpy as np
import pytest
import torch

from conftest import golden, rnd
from oracle import ldm_oracle as O

SCALE = 0.18215
T = lambda a: torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def g20():
    return golden("g20_kl.npz")


def configs():
    from dsml_thesis_amd import synth
    return dict(f4=(synth.KL_F4, 128), f8=(synth.KL_F8_SMALL, 64))


def recorded_shapes(g20, tag):
    return {str(k): tuple(int(d) for d in str(s).split(",")) for k, s in zip(g20[f"{tag}_keys"], g20[f"{tag}_shapes"])}


def test_factory_resolves_both_targets():
    from dsml_thesis_amd import autoencoder as A, synth
    from dsml_thesis_amd.util import get_obj_from_str, instantiate_from_config
    assert get_obj_from_str("ldm.models.autoencoder.AutoencoderKL") is A.AutoencoderKL
    assert get_obj_from_str("ldm.models.autoencoder.IdentityFirstStage") is A.IdentityFirstStage
    fs = instantiate_from_config(synth.kl_config(kl=synth.KL_F8_SMALL)["first_stage_config"])
    assert isinstance(fs, A.AutoencoderKL) and fs.embed_dim == 4
    ident = instantiate_from_config(dict(target="ldm.models.autoencoder.IdentityFirstStage", params=dict(vq_interface=True)))
    x = rnd(1, 2, 3, 4, 4)
    assert ident.encode(x) is x and ident.decode(x, "extra", k=1) is x and ident(x) is x
    q = ident.quantize(x)
    assert q[0] is x and q[1] is None and list(q[2]) == [None, None, None]
    plain = A.IdentityFirstStage()
    assert plain.quantize(x) is x and plain.vq_interface is False and len(list(plain.parameters())) == 0


@pytest.mark.parametrize("tag", ["f4", "f8"])
def test_parameter_tree_equals_the_reference(g20, tag):
    from dsml_thesis_amd.autoencoder import AutoencoderKL
    kl, _ = configs()[tag]
    fs = AutoencoderKL(dict(kl["ddconfig"]), dict(target="torch.nn.Identity"), kl["embed_dim"])
    mine = [(k, tuple(v.shape)) for k, v in fs.state_dict().items()]
    assert mine == list(recorded_shapes(g20, tag).items())
    e, z = kl["embed_dim"], kl["ddconfig"]["z_channels"]
    assert tuple(fs.quant_conv.weight.shape) == (2 * e, 2 * z, 1, 1) and tuple(fs.post_quant_conv.weight.shape) == (z, e, 1, 1)


def test_refusals_need_no_gpu():
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.autoencoder import AutoencoderKL
    from dsml_thesis_amd.ddpm import LatentDiffusion
    from dsml_thesis_amd.distributions import DiagonalGaussianDistribution
    from dsml_thesis_amd.latent_diffclip import LatentDiffusionCLIP
    from dsml_thesis_amd.latent_tune import LatentDiffusionTune
    loss = dict(target="torch.nn.Identity")
    for kl in (synth.KL_F4, synth.KL_F8_SMALL):
        with pytest.raises(AssertionError):
            AutoencoderKL(dict(kl["ddconfig"], double_z=False), loss, kl["embed_dim"])
    with pytest.raises(NotImplementedError, match="z_channels <= 4"):
        AutoencoderKL(dict(synth.KL_F8_SMALL["ddconfig"], z_channels=16), loss, 4)
    with pytest.raises(NotImplementedError, match="embed_dim <= 4"):
        AutoencoderKL(dict(synth.KL_F8_SMALL["ddconfig"]), loss, 16)
    small = dict(synth.FR_UNET, model_channels=32, channel_mult=[1], num_res_blocks=1, attention_resolutions=[])
    cfg = synth.kl_config(unet=small, kl=synth.KL_F8_SMALL)
    cfg["unet_config"]["params"].update(in_channels=4, out_channels=4)
    m = LatentDiffusion(**cfg)
    assert m.scale_factor == SCALE and m.restarted_from_ckpt is False
    with pytest.raises(NotImplementedError, match="not yet implemented"):
        m.get_first_stage_encoding([1, 2])
    x = rnd(2, 1, 4, 8, 8)
    torch.testing.assert_close(m.get_first_stage_encoding(x), SCALE * x, rtol=0, atol=0)
    m.split_input_params = dict(ks=(8, 8), stride=(4, 4), vqf=8, patch_distributed_vq=True)
    with pytest.raises(NotImplementedError, match="AutoencoderKL"):
        m.encode_first_stage(rnd(3, 1, 3, 64, 64))
    del m.split_input_params
    t = torch.zeros(1, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="no `quantize`"):
        m._quantize_denoised(x)
    m.apply_model = lambda x_, t_, c_: x_                      # (the refusal sits behind the UNet evaluation)
    with pytest.raises(NotImplementedError, match="quantize_denoised"):
        m.p_mean_variance(x, None, t, clip_denoised=False, quantize_denoised=True)
    with pytest.raises(AssertionError, match="std-rescaling"):   # custom scale_factor and scale_by_std together
        m2 = LatentDiffusion(**dict(cfg, scale_by_std=True))
        m2.on_train_batch_start(dict(image=rnd(4, 1, 64, 64, 3)), 0, 0)
    with pytest.raises(NotImplementedError, match="VQ first stage"):
        LatentDiffusionCLIP(cfg["first_stage_config"], cfg["cond_stage_config"], edit_attr="happy",
                            **{k: v for k, v in cfg.items() if k not in ("first_stage_config", "cond_stage_config")})
    from dsml_thesis_amd.synth import tf_config
    tcfg = tf_config()
    tcfg["first_stage_config"] = synth.kl_config()["first_stage_config"]
    with pytest.raises(NotImplementedError, match="VQ first stage"):
        LatentDiffusionTune(**tcfg)
    with pytest.raises(Exception, match="CUDA tensors only"):
        DiagonalGaussianDistribution(rnd(5, 1, 4, 2, 2)).sample()


@pytest.mark.parametrize("tag", ["f4", "f8"])
def test_oracle_reproduces_the_fixture(g20, tag):
    """The oracle's encoder / decoder with a double_z ddconfig and the recipe weights are the CPU yardstick for g20."""
    from dsml_thesis_amd.synth import synth_state_dict
    kl, res = configs()[tag]
    sd = synth_state_dict(recorded_shapes(g20, tag))
    moments = O.encode_first_stage(sd, kl, rnd(201, 2, 3, res, res))
    torch.testing.assert_close(moments, T(g20[f"{tag}_moments"]), rtol=1e-5, atol=1e-5)
    q = torch.nn.functional.conv2d(T(g20[f"{tag}_z"]) / SCALE, sd["post_quant_conv.weight"], sd["post_quant_conv.bias"])
    torch.testing.assert_close(O.decoder_forward(sd, kl["ddconfig"], q), T(g20[f"{tag}_decoded"]), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("tag", ["f4", "f8"])
def test_kl_and_nll_on_cpu_tensors(g20, tag):
    from dsml_thesis_amd.distributions import DiagonalGaussianDistribution, normal_kl
    post = DiagonalGaussianDistribution(T(g20[f"{tag}_moments"]))
    e = post.parameters.shape[1] // 2
    assert torch.equal(post.mean, post.parameters[:, :e]) and post.mode() is post.mean and post.deterministic is False
    assert torch.equal(post.logvar, post.parameters[:, e:].clamp(-30.0, 20.0))
    assert torch.equal(post.std, torch.exp(0.5 * post.logvar)) and torch.equal(post.var, torch.exp(post.logvar))
    torch.testing.assert_close(post.kl(), T(g20[f"{tag}_kl"]), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(post.nll(T(g20[f"{tag}_z"])), T(g20[f"{tag}_nll"]), rtol=1e-5, atol=1e-5)
    # kl against another posterior, and normal_kl, from the closed form in float64
    other = DiagonalGaussianDistribution(rnd(7, *post.parameters.shape) * 0.5)
    m1, l1, m2, l2 = (t.double() for t in (post.mean, post.logvar, other.mean, other.logvar))
    want = 0.5 * (-1.0 + l2 - l1 + torch.exp(l1 - l2) + (m1 - m2) ** 2 * torch.exp(-l2))
    torch.testing.assert_close(post.kl(other).double(), want.sum(dim=[1, 2, 3]), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(normal_kl(post.mean, post.logvar, other.mean, other.logvar).double(), want, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(normal_kl(post.mean, post.logvar, 0.0, 0.0).sum(dim=[1, 2, 3]), post.kl(), rtol=1e-5, atol=1e-5)
    det = DiagonalGaussianDistribution(post.parameters, deterministic=True)
    assert not det.std.any() and not det.var.any() and float(det.kl()) == 0.0 and float(det.nll(post.mean)) == 0.0


def test_entry_points_validate_before_any_launch():
    from dsml_thesis_amd import lib as L
    lib = L.load()
    p = 4096                                                     # never dereferenced: validation precedes any launch
    ok = dict(n=1, h=4, w=4, cin=64, c2z=6, c2e=6)

    def head(**over):
        a = dict(ok, **over)
        return lib.ldmk_conv3x3_moments(p, p, p, p, p, p, p, a["n"], a["h"], a["w"], a["cin"], a["c2z"], a["c2e"], None)

    for over, msg in ((dict(c2z=5), b"c2z=5"), (dict(c2z=10), b"c2z=10"), (dict(cin=6), b"cin=6"), (dict(c2e=3), b"c2e=3"),
                      (dict(c2e=12), b"c2e=12"), (dict(c2z=0), b"c2z=0"), (dict(h=0), b"bad args")):
        assert head(**over) == -1 and msg in lib.ldmk_last_error(), (over, lib.ldmk_last_error())
    assert lib.ldmk_gauss_posterior(p, None, 1.0, None, None, None, None, 1, 3, 16, None) == -1
    assert b"no output" in lib.ldmk_last_error()
    assert lib.ldmk_gauss_posterior(p, p, 1.0, p, None, None, None, 1, 3, 16, None) == -1
    assert b"noise without z" in lib.ldmk_last_error()
    assert lib.ldmk_gauss_posterior(p, None, 1.0, p, None, None, None, 1, 0, 16, None) == -1
