"""Synthetic-weight models for benchmarks, tools and smoke runs (no checkpoints exist offline).

Shipped hyper-parameters (values restated from face_reenactment/configs/latent-diffusion/affectnet-128-ldm-vq-f4.yaml:18-62
and talking_face/configs/latent-diffusion/mead-128-ldm-f4.yaml:19-63) and the SURVEY §8(c) weight recipe
`RandomState(crc32(key) ^ seed)`.  The oracle keeps its own copy of both (oracle/weights.py is test infrastructure and
is never imported from here); tests/test_host_logic.py checks that the two agree bit for bit."""
import zlib
from collections import OrderedDict

import numpy as np
import torch

FR_UNET = dict(image_size=32, in_channels=3, out_channels=3, model_channels=160, attention_resolutions=[4, 2, 1],
               num_res_blocks=2, channel_mult=[1, 2, 4], num_head_channels=32, use_spatial_transformer=True,
               transformer_depth=1, context_dim=512)
TF_UNET = dict(FR_UNET, in_channels=9, context_dim=1024)
NS_UNET = dict(FR_UNET, image_size=64, in_channels=4, out_channels=4)          # north-star 64x64x4 latent
# BASELINE configs[0] as worded: a genuinely unconditional LDM -- no SpatialTransformer / context, AttentionBlock with 32-channel heads
UNCOND_UNET = dict(image_size=64, in_channels=4, out_channels=4, model_channels=160, attention_resolutions=[4, 2, 1],
                   num_res_blocks=2, channel_mult=[1, 2, 4], num_head_channels=32)
# class-conditional ('adm') UNet with the shipped UNet's widths (160 / 320 / 640 channels, two ResBlocks per level): scale-shift norm,
# label embedding, AttentionBlock / QKVAttention -- the training benchmark's third model (tools/train_bench.py --unet adm); its
# GroupNorm shapes are the shipped UNet's, so the FiLM backward can be timed next to the plain one
ADM_TRAIN_UNET = dict(image_size=32, in_channels=3, out_channels=3, model_channels=160, attention_resolutions=[4, 2, 1],
                      num_res_blocks=2, channel_mult=[1, 2, 4], num_head_channels=32, use_scale_shift_norm=True, num_classes=1000,
                      use_new_attention_order=True)
VQ_F4 = dict(embed_dim=3, n_embed=16384,
             ddconfig=dict(double_z=False, z_channels=3, resolution=128, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4],
                           num_res_blocks=2, attn_resolutions=[32], dropout=0.0))
VQ_F4_256 = dict(embed_dim=4, n_embed=16384,
                 ddconfig=dict(double_z=False, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128,
                               ch_mult=[1, 2, 4], num_res_blocks=2, attn_resolutions=[64], dropout=0.0))
# KL-regularised first stages (ldm.models.autoencoder.AutoencoderKL): KL-f4 with the VQ-f4 trunk, and a narrow four-level KL-f8
KL_F4 = dict(embed_dim=3, ddconfig=dict(VQ_F4["ddconfig"], double_z=True))
KL_F8_SMALL = dict(embed_dim=4,
                   ddconfig=dict(double_z=True, z_channels=4, resolution=64, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 2, 4],
                                 num_res_blocks=1, attn_resolutions=[], dropout=0.0))
# first-stage training tests: a two-level VQGAN with attention at the latent resolution, 64 codes (2.80 M parameters)
VQ_TRAIN_SMALL = dict(embed_dim=3, n_embed=64,
                      ddconfig=dict(double_z=False, z_channels=3, resolution=32, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2],
                                    num_res_blocks=1, attn_resolutions=[16], dropout=0.0))
# the KL sibling: the same trunk with a 6-channel moment head (z_channels = embed_dim = 3)
KL_TRAIN_SMALL = dict(embed_dim=3, ddconfig=dict(VQ_TRAIN_SMALL["ddconfig"], double_z=True))
SCHEDULE = dict(timesteps=1000, linear_start=0.0015, linear_end=0.0205)


def synth_tensor(key, shape, seed=0, gain=1.0):
    """weights with >= 2 dims: N(0,1)/sqrt(fan_in)*gain (embedding tables: plain N(0,1)); biases: 0.02*N(0,1);
    1-D norm weights: 1 + 0.1*N(0,1).  MT19937 `RandomState` is bit-stable across NumPy versions and machines."""
    rs = np.random.RandomState((zlib.crc32(key.encode()) ^ seed) & 0xFFFFFFFF)
    n = rs.standard_normal(tuple(shape)).astype(np.float32)
    if len(shape) >= 2:
        if key.endswith("embedding.weight"):
            return n
        return (n * np.float32(gain / np.sqrt(int(np.prod(shape[1:]))))).astype(np.float32)
    if key.endswith(".bias"):
        return (n * np.float32(0.02)).astype(np.float32)
    return (np.float32(1.0) + np.float32(0.1) * n).astype(np.float32)


def synth_state_dict(shapes, seed=0, gain=1.0):
    return OrderedDict((k, torch.from_numpy(synth_tensor(k, s, seed=seed, gain=gain))) for k, s in shapes.items())


def load_recipe(module, gain=1.0, seed=0):
    """Fill every floating-point tensor of `module` from the recipe, keyed by its own state-dict names."""
    sd = module.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items() if v.dtype.is_floating_point and v.dim() > 0}
    new = synth_state_dict(shapes, seed=seed, gain=gain)
    module.load_state_dict(new, strict=False)
    return new


# VGG16 `features` indices of the thirteen convolutions per LPIPS slice, with (cin, cout): the reference's `net.slice{k}.{i}` keys
LPIPS_VGG = ((1, ((0, 3, 64), (2, 64, 64))), (2, ((5, 64, 128), (7, 128, 128))), (3, ((10, 128, 256), (12, 256, 256), (14, 256, 256))),
             (4, ((17, 256, 512), (19, 512, 512), (21, 512, 512))), (5, ((24, 512, 512), (26, 512, 512), (28, 512, 512))))
LPIPS_CHNS = (64, 128, 256, 512, 512)
LPIPS_SHIFT, LPIPS_SCALE = (-.030, -.088, -.188), (.458, .448, .450)


def lpips_state_dict(seed=0, use_dropout=True):
    """A synthetic LPIPS state dict with the reference's keys (taming/modules/losses/lpips.py), drawn in key order from ONE
    RandomState(seed): convolution weights He-normal N(0, sqrt(2 / (9 cin))), biases N(0, 0.05), lin weights U(0, 1); the
    ScalingLayer buffers hold their constants.  14.7 M parameters: generated where they are needed, never stored in a fixture."""
    rs = np.random.RandomState(seed)
    sd = OrderedDict()
    sd["scaling_layer.shift"] = torch.tensor(LPIPS_SHIFT, dtype=torch.float32)[None, :, None, None]
    sd["scaling_layer.scale"] = torch.tensor(LPIPS_SCALE, dtype=torch.float32)[None, :, None, None]
    for k, convs in LPIPS_VGG:
        for i, cin, cout in convs:
            w = rs.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))
            sd[f"net.slice{k}.{i}.weight"] = torch.from_numpy(w.astype(np.float32))
            sd[f"net.slice{k}.{i}.bias"] = torch.from_numpy((rs.standard_normal(cout) * 0.05).astype(np.float32))
    for k, c in enumerate(LPIPS_CHNS):
        sd[f"lin{k}.model.{1 if use_dropout else 0}.weight"] = torch.from_numpy(rs.uniform(0.0, 1.0, (1, c, 1, 1)).astype(np.float32))
    return sd


def fr_config(unet=None, vq=None):
    unet, vq = unet or FR_UNET, vq or VQ_F4
    return dict(
        first_stage_config=dict(target="ldm.models.autoencoder.VQModelInterface",
                                params=dict(embed_dim=vq["embed_dim"], n_embed=vq["n_embed"], ddconfig=dict(vq["ddconfig"]),
                                            lossconfig=dict(target="torch.nn.Identity"))),
        cond_stage_config=dict(target="ldm.modules.encoders.modules.ClassEmbedder3",
                               params=dict(embed_dim=512, n_classes=8, key="class_label", p_uncond=0.2)),
        unet_config=dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(unet)),
        num_timesteps_cond=1, cond_stage_key="class_label", cond_stage_trainable=True, conditioning_key="crossattn",
        image_size=unet["image_size"], channels=unet["out_channels"], first_stage_key="image", log_every_t=200,
        monitor="val_loss_ema", **SCHEDULE)


def uncond_config(unet=None, vq=None):
    """cond_stage_config '__is_unconditional__' -> conditioning_key None (ddpm.py:443-444): DiffusionWrapper calls the UNet as
    diffusion_model(x, t)."""
    cfg = fr_config(unet or UNCOND_UNET, vq or VQ_F4_256)
    cfg.update(cond_stage_config="__is_unconditional__", cond_stage_trainable=False, conditioning_key=None)
    return cfg


def make_uncond_model(gain=1.0, unet=None, vq=None, device="cuda"):
    from .ddpm import LatentDiffusion
    m = LatentDiffusion(**uncond_config(unet, vq))
    load_recipe(m.model.diffusion_model, gain=gain)
    load_recipe(m.first_stage_model)
    return m.to(device).eval()


def tf_config(seq_len=17):
    return dict(
        first_stage_config=fr_config()["first_stage_config"],
        cond_stage_config_1=dict(target="ldm.modules.encoders.modules.ClassEmbedder",
                                 params=dict(embed_dim=256, n_classes=8, key="class_label", p_uncond=0.2)),
        cond_stage_config_2=dict(target="ldm.modules.encoders.modules.Conv1DTemporalAttention",
                                 params=dict(seq_len=seq_len, subspace_dim=768, subspace2hidden=False)),
        unet_config=dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(TF_UNET)),
        num_timesteps_cond=1, cond_stage_key_1="class_label", cond_stage_key_2="audio", cond_stage_trainable=True,
        conditioning_key="crossattn", image_size=32, channels=3, first_stage_key="image", log_every_t=200,
        monitor="val_loss_ema", **SCHEDULE)


def kl_config(unet=None, kl=None, scale_factor=0.18215, scale_by_std=False):
    """fr_config with an AutoencoderKL first stage (the `scale_factor` the published KL checkpoints ship with)."""
    kl = kl or KL_F4
    cfg = fr_config(unet)
    cfg.update(first_stage_config=dict(target="ldm.models.autoencoder.AutoencoderKL",
                                       params=dict(embed_dim=kl["embed_dim"], ddconfig=dict(kl["ddconfig"]),
                                                   lossconfig=dict(target="torch.nn.Identity"))),
               scale_factor=scale_factor, scale_by_std=scale_by_std)
    return cfg


def make_kl_model(gain=1.0, scale_factor=0.18215, unet=None, kl=None, scale_by_std=False, device="cuda"):
    from .ddpm import LatentDiffusion
    m = LatentDiffusion(**kl_config(unet, kl, scale_factor, scale_by_std))
    load_recipe(m.model.diffusion_model, gain=gain)
    load_recipe(m.first_stage_model)
    load_recipe(m.cond_stage_model)
    return m.to(device).eval()


def make_vq_first_stage(vq=None, seed=0, device="cuda"):
    """A stand-alone VQ first stage with recipe weights (what train_first_stage.FirstStageTrainer wraps)."""
    from .autoencoder import VQModelInterface
    vq = vq or VQ_TRAIN_SMALL
    m = VQModelInterface(embed_dim=vq["embed_dim"], n_embed=vq["n_embed"], ddconfig=dict(vq["ddconfig"]),
                         lossconfig=dict(target="torch.nn.Identity"))
    load_recipe(m, seed=seed)
    return m.to(device).eval()


def make_kl_first_stage(kl=None, seed=0, device="cuda"):
    """A stand-alone KL first stage with recipe weights (the KL kind of train_first_stage.FirstStageTrainer)."""
    from .autoencoder import AutoencoderKL
    kl = kl or KL_TRAIN_SMALL
    m = AutoencoderKL(embed_dim=kl["embed_dim"], ddconfig=dict(kl["ddconfig"]), lossconfig=dict(target="torch.nn.Identity"))
    load_recipe(m, seed=seed)
    return m.to(device).eval()


def make_fr_model(gain=1.0, unet=None, vq=None, device="cuda"):
    from .ddpm import LatentDiffusion
    m = LatentDiffusion(**fr_config(unet, vq))
    load_recipe(m.model.diffusion_model, gain=gain)
    load_recipe(m.first_stage_model)
    load_recipe(m.cond_stage_model)
    return m.to(device).eval()


def make_tf_model(gain=1.0, seq_len=17, device="cuda"):
    from .ddpm import LatentDiffusion2Cond
    m = LatentDiffusion2Cond(**tf_config(seq_len))
    load_recipe(m.model.diffusion_model, gain=gain)
    load_recipe(m.first_stage_model)
    load_recipe(m.cond_stage_model_1)
    load_recipe(m.cond_stage_model_2)
    return m.to(device).eval()
