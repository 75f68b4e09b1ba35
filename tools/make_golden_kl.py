"""Generate tests/golden/g20_kl.npz and g20_kl_patch.npz from the REAL face-reenactment reference (container only, CPU).

Usage (from the repository root):   python tools/make_golden_kl.py

An `AutoencoderKL` first stage (autoencoder.py:285-342) under the reference `LatentDiffusion(scale_factor=0.18215)`, with
the recipe weights `synth.load_recipe` gives the native classes, for two configurations: KL-f4 on the VQ-f4 trunk
(`synth.KL_F4`, prefix `f4_`) and a narrow four-level KL-f8 (`synth.KL_F8_SMALL`, prefix `f8_`).  Per configuration:
the state-dict key list with shapes, the encoder's moments, the posterior sample under a fixed seed together with the
noise it drew, the decoded image, `kl()` / `nll(z)`, a patch-wise decode, and the `scale_by_std` rescaling of
`on_train_batch_start`.  Only recorded arrays and lists of names / shapes are stored.  The two patch-wise decodes are the
largest arrays and go to a file of their own so that each file stays under the 1 MiB a committed file may have.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import weights as W  # noqa: E402
from tools.make_golden import load_recipe, rnd, save  # noqa: E402
from tools.make_golden_split import SPLIT  # noqa: E402

KL_F4 = dict(embed_dim=3, ddconfig=dict(W.VQ_F4["ddconfig"], double_z=True))
KL_F8_SMALL = dict(embed_dim=4,
                   ddconfig=dict(double_z=True, z_channels=4, resolution=64, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 2, 4],
                                 num_res_blocks=1, attn_resolutions=[], dropout=0.0))
SCALE = 0.18215
# patch-wise decode: (latent h, w, split parameters).  f4: g19's geometry (Ly = 2, Lx = 3); f8: the same grid at its latent size
PATCH = dict(f4=(48, 64, dict(SPLIT)), f8=(12, 16, dict(SPLIT, ks=(8, 8), stride=(4, 4), vqf=8)))
SEED_Z, SEED_STD = 11, 12


def build(kl, **kw):
    from ldm.models.diffusion.ddpm import LatentDiffusion
    fs_cfg = dict(target="ldm.models.autoencoder.AutoencoderKL",
                  params=dict(embed_dim=kl["embed_dim"], ddconfig=dict(kl["ddconfig"]), lossconfig=dict(target="torch.nn.Identity")))
    unet = dict(W.FR_UNET, in_channels=kl["embed_dim"], out_channels=kl["embed_dim"])
    ld = LatentDiffusion(first_stage_config=fs_cfg, cond_stage_config="__is_unconditional__", num_timesteps_cond=1,
                         unet_config=dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=unet),
                         image_size=32, channels=kl["embed_dim"], first_stage_key="image", monitor="val_loss_ema",
                         **W.SCHEDULE, **kw)
    load_recipe(ld.first_stage_model, seed=0)
    return ld.eval()


def gen_one(tag, kl, res, g, gp):
    from ldm.modules.distributions.distributions import DiagonalGaussianDistribution
    ld = build(kl, scale_factor=SCALE)
    fs = ld.first_stage_model
    sd = fs.state_dict()
    g[f"{tag}_keys"] = np.array(list(sd.keys()))
    g[f"{tag}_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    x = rnd(201, 2, 3, res, res)
    post = ld.encode_first_stage(x)
    assert isinstance(post, DiagonalGaussianDistribution)
    g[f"{tag}_moments"] = post.parameters
    torch.manual_seed(SEED_Z)
    g[f"{tag}_noise"] = torch.randn(post.mean.shape)
    torch.manual_seed(SEED_Z)
    z = ld.get_first_stage_encoding(post)
    assert torch.equal(z, SCALE * (post.mean + post.std * g[f"{tag}_noise"]))
    g[f"{tag}_z"] = z
    g[f"{tag}_decoded"] = ld.decode_first_stage(z)
    g[f"{tag}_kl"], g[f"{tag}_nll"] = post.kl(), post.nll(z)
    h, w, split = PATCH[tag]
    ld.split_input_params = dict(split)
    gp[f"{tag}_patch_decoded"] = ld.decode_first_stage(rnd(204, 1, kl["embed_dim"], h, w))
    if tag == "f4":                          # the patch-wise ENCODE of a KL first stage fails in the reference (ddpm.py:851)
        try:
            ld.encode_first_stage(rnd(205, 1, 3, 128, 128))
            raise AssertionError("expected the reference's patch-wise KL encode to fail")
        except TypeError as e:
            print(f"  [{tag}] patch-wise encode raises TypeError: {str(e)[:60]}")
    # scale_by_std: the first batch of a fresh run sets scale_factor = 1 / std(latents)
    ld2 = build(kl, scale_factor=1.0, scale_by_std=True)
    ld2.current_epoch, ld2.global_step = 0, 0
    batch = dict(image=x.permute(0, 2, 3, 1).contiguous())
    torch.manual_seed(SEED_STD)
    g[f"{tag}_std_noise"] = torch.randn(post.mean.shape)
    torch.manual_seed(SEED_STD)
    ld2.on_train_batch_start(batch, 0, 0)
    g[f"{tag}_std_scale_factor"] = ld2.scale_factor
    assert torch.allclose(ld2.scale_factor, 1. / (post.mean + post.std * g[f"{tag}_std_noise"]).flatten().std())


def gen_kl():
    from tools import ref_shims
    ref_shims.install("face_reenactment")
    torch.set_grad_enabled(False)
    g, gp = {}, {}
    gen_one("f4", KL_F4, 128, g, gp)
    gen_one("f8", KL_F8_SMALL, 64, g, gp)
    for d in (g, gp):
        for k, v in d.items():
            if isinstance(v, torch.Tensor):
                assert torch.isfinite(v).all(), k
                print(f"  {k:22s} {tuple(v.shape)}  max|.| {v.abs().max().item():.4g}")
    save("g20_kl.npz", **g)
    save("g20_kl_patch.npz", **gp)


if __name__ == "__main__":
    gen_kl()
