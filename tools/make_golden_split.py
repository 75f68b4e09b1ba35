"""Generate tests/golden/g19_split.npz from the REAL face-reenactment reference (container only, CPU).

Usage (from the repository root):   python tools/make_golden_split.py

The patch-wise mode of `LatentDiffusion` (ddpm.py:565-652 weighting / fold / unfold, :716-753 decode, :828-859 encode,
:904-986 apply_model): the reference class with `split_input_params` set, the recipe weights of `make_fr_model(gain=0.25)`
and seeded inputs.  Ly = 2, Lx = 3 at the latent size 48x64, so a transposed patch index cannot reproduce any of it.
Only recorded arrays are stored.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import weights as W  # noqa: E402
from tools.make_golden import load_recipe, rnd, save  # noqa: E402

SPLIT = dict(ks=(32, 32), stride=(16, 16), vqf=4, patch_distributed_vq=True, tie_braker=False, clip_min_weight=0.01,
             clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
H, W_ = 48, 64


def gen_split():
    from tools import ref_shims
    ref_shims.install("face_reenactment")
    from ldm.models.diffusion.ddim import DDIMSampler
    from ldm.models.diffusion.ddpm import LatentDiffusion
    torch.set_grad_enabled(False)
    unet_cfg = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(W.FR_UNET))
    fs_cfg = dict(target="ldm.models.autoencoder.VQModelInterface",
                  params=dict(embed_dim=3, n_embed=16384, ddconfig=dict(W.VQ_F4["ddconfig"]),
                              lossconfig=dict(target="torch.nn.Identity")))
    cond_cfg = dict(target="ldm.modules.encoders.modules.ClassEmbedder3",
                    params=dict(embed_dim=512, n_classes=8, key="class_label", p_uncond=0.2))
    ld = LatentDiffusion(first_stage_config=fs_cfg, cond_stage_config=cond_cfg, num_timesteps_cond=1,
                         cond_stage_key="class_label", cond_stage_trainable=True, conditioning_key="crossattn",
                         unet_config=unet_cfg, image_size=32, channels=3, first_stage_key="image", log_every_t=200,
                         monitor="val_loss_ema", **W.SCHEDULE)
    load_recipe(ld.model.diffusion_model, seed=0, gain=0.25, prefix_check=W.unet_param_shapes(W.FR_UNET))
    load_recipe(ld.first_stage_model, seed=0, prefix_check=W.vqmodel_param_shapes(W.VQ_F4))
    load_recipe(ld.cond_stage_model, seed=0)
    ld.eval()
    ld.split_input_params = dict(SPLIT)
    g = {}

    def geometry(tag, x, **kw):
        _, _, norm, weight = ld.get_fold_unfold(x, SPLIT["ks"], SPLIT["stride"], **kw)
        g["weight" + tag] = weight[0, 0]                          # [kh][kw][L]
        g["norm" + tag] = norm[0, 0]                              # [h][w]
        print(f"  geometry{tag or '_latent'}: weight {tuple(weight.shape[2:])} norm {tuple(norm.shape[2:])}")

    print("[G19] fold geometries")
    geometry("", torch.zeros(1, 3, H, W_))
    geometry("_dec", torch.zeros(1, 3, H, W_), uf=SPLIT["vqf"])
    geometry("_enc", torch.zeros(1, 3, 4 * H, 4 * W_), df=SPLIT["vqf"])
    ld.split_input_params["tie_braker"] = True
    _, _, norm, weight = ld.get_fold_unfold(torch.zeros(1, 3, 16, 16), (8, 8), (4, 4))
    g["weight_tie"], g["norm_tie"] = weight[0, 0], norm[0, 0]
    ld.split_input_params["tie_braker"] = False

    print("[G19] apply_model")
    labels = torch.tensor([1, 6])
    c = ld.cond_stage_model.embedding(labels[:, None])
    uc = ld.cond_stage_model.uncond_embedding(torch.zeros(2, 1, dtype=torch.long))
    x, t = rnd(191, 2, 3, H, W_), torch.tensor([137, 842])
    g["eps"] = ld.apply_model(x, t, c)

    class CPUDDIM(DDIMSampler):          # the reference hard-codes .to('cuda')
        def register_buffer(self, n, a):
            setattr(self, n, a)

    print("[G19] DDIMSampler.sample S=4")
    sampler = CPUDDIM(ld)
    xT = rnd(192, 2, 3, H, W_)
    g["sample_S4"], _ = sampler.sample(S=4, batch_size=2, shape=[3, H, W_], conditioning=c, eta=0.0, x_T=xT, verbose=False)
    g["sample_S4_cfg"], _ = sampler.sample(S=4, batch_size=2, shape=[3, H, W_], conditioning=c, eta=0.0, x_T=xT, verbose=False,
                                           unconditional_guidance_scale=3.0, unconditional_conditioning=uc)

    print("[G19] first stage")
    g["decoded_noquant"] = ld.decode_first_stage(rnd(193, 1, 3, H, W_), force_not_quantize=True)
    g["encoded"] = ld.encode_first_stage(rnd(194, 1, 3, 4 * H, 4 * W_))
    assert tuple(ld.split_input_params["original_image_size"]) == (4 * H, 4 * W_)
    for k, v in g.items():
        assert torch.isfinite(v).all(), k
        print(f"  {k:18s} {tuple(v.shape)}  max|.| {v.abs().max().item():.4g}")
    save("g19_split.npz", **g)


if __name__ == "__main__":
    gen_split()
