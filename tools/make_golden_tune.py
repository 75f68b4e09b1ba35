"""Generate tests/golden/g18_tune.npz from the REAL talking-face reference (container only, CPU).

Usage (from the repository root):   python tools/make_golden_tune.py

The talking-face fine-tune (ddpm2condtune.py:947-1112) cannot be imported: the module loads the lip-reading package at
import.  Everything it runs up to the decoded image lives in classes that do import -- `ddim2cond.DDIMSampler.
differentiable_stochastic_encode / differentiable_decode` with `make_schedule(8, ddim_eta=1.0)` (ddpm2condtune.py:533,
1028-1032) and `ddpm2cond.LatentDiffusion.apply_model / differentiable_decode_first_stage` (the same methods as in the tune
file) -- so this drives those with the loop of `forward` + `p_losses`, the sampler's `noise_like` replaced by recorded seeded
draws, and autograd for the gradients.  The lip-reading term is `lip_loss` below: a small fixed function that exists only so
that an image-space gradient with a spatial mask flows through the clamp; tests/test_tune_gpu.py repeats it verbatim.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import weights as W  # noqa: E402
from tools.make_golden import load_recipe, rnd, save  # noqa: E402

SEQ_LEN, N, HW, STEPS = 9, 2, 16, 8


def lip_loss(x, x0, l):
    """1 - mean cosine similarity of a seeded 3x3 conv + mean-pool feature of a fixed mouth-region crop (64x64 frames)."""
    w = (0.2 * rnd(620, 8, 3, 3, 3)).to(x.device, x.dtype)

    def feat(im):
        return F.avg_pool2d(F.conv2d(im[:, :, 36:60, 16:48], w), 4).flatten(1)
    a, b = feat(x0), feat(x)
    lr = (a * b).sum(1) / torch.linalg.norm(b, dim=1) / torch.linalg.norm(a, dim=1)
    return 1 - torch.mean(lr)


def gen_tune():
    from tools import ref_shims
    ref_shims.install("talking_face")
    import ldm.models.diffusion.ddim2cond as ddim2cond
    from ldm.models.diffusion.ddpm2cond import LatentDiffusion
    unet_cfg = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(W.TF_UNET))
    fs_cfg = dict(target="ldm.models.autoencoder.VQModelInterface",
                  params=dict(embed_dim=3, n_embed=16384, ddconfig=dict(W.VQ_F4["ddconfig"]),
                              lossconfig=dict(target="torch.nn.Identity")))
    c1_cfg = dict(target="ldm.modules.encoders.modules.ClassEmbedder",
                  params=dict(embed_dim=256, n_classes=8, key="class_label", p_uncond=0.0))
    c2_cfg = dict(target="ldm.modules.encoders.modules.Conv1DTemporalAttention",
                  params=dict(seq_len=SEQ_LEN, subspace_dim=768, subspace2hidden=False))
    ld = LatentDiffusion(first_stage_config=fs_cfg, cond_stage_config_1=c1_cfg, cond_stage_config_2=c2_cfg,
                         num_timesteps_cond=1, cond_stage_key_1="class_label", cond_stage_key_2="audio",
                         cond_stage_trainable=True, conditioning_key="crossattn", unet_config=unet_cfg,
                         image_size=HW, channels=3, first_stage_key="image", log_every_t=200,
                         monitor="val_loss_ema", **W.SCHEDULE)
    unet = ld.model.diffusion_model
    load_recipe(unet, seed=0, gain=0.25, prefix_check=W.unet_param_shapes(W.TF_UNET))
    load_recipe(ld.first_stage_model, seed=0, prefix_check=W.vqmodel_param_shapes(W.VQ_F4))
    load_recipe(ld.cond_stage_model_1, seed=0)
    load_recipe(ld.cond_stage_model_2, seed=0, prefix_check=W.audio_attention_param_shapes(SEQ_LEN))
    ld.train()
    for m in (unet, ld.cond_stage_model_1, ld.cond_stage_model_2):
        for p_ in m.parameters():
            p_.requires_grad_(True)

    class CPUDDIM(ddim2cond.DDIMSampler):
        def register_buffer(self, n, a):
            setattr(self, n, a)

    sm = CPUDDIM(ld)
    sm.make_schedule(ddim_num_steps=STEPS, ddim_eta=1.0, verbose=False)
    torch.set_grad_enabled(True)
    x_start, q_noise = rnd(601, N, 3, HW, HW), rnd(602, N, 3, HW, HW)
    c3, c4 = rnd(603, N, 3, HW, HW), rnd(604, N, 3, HW, HW)
    window = rnd(605, N, SEQ_LEN, 768)
    labels = torch.tensor([2, 6])
    landmarks = torch.zeros(N, 20, 2)
    t = torch.tensor([137, 842])
    draws = [rnd(610 + i, N, 3, HW, HW) for i in range(STEPS)]
    queue = list(draws)
    real_noise_like = ddim2cond.noise_like
    ddim2cond.noise_like = lambda shape, device, repeat=False: queue.pop(0)
    try:
        c1 = ld.cond_stage_model_1({"class_label": labels}, training=False)
        c2 = ld.cond_stage_model_2(window)
        c12 = torch.cat([c1, c2], dim=2)
        c12.retain_grad()
        c34 = torch.cat([c3, c4], dim=1)
        x_noisy = sm.differentiable_stochastic_encode(x_start, t, use_original_steps=True, noise=q_noise)
        x_recon = sm.differentiable_decode(x_noisy, {"class_label_&_audio": c12, "motion_&_id": c34}, t_start=1000,
                                           use_original_steps=False)
    finally:
        ddim2cond.noise_like = real_noise_like
    assert not queue
    decoded = ld.differentiable_decode_first_stage(x_recon)
    x = torch.clamp(decoded, min=-1.0, max=1.0)
    x0 = torch.clamp(ld.differentiable_decode_first_stage(x_start), min=-1.0, max=1.0)
    lr_loss = lip_loss(x, x0, landmarks)
    l2_loss = torch.nn.MSELoss()(x_recon, x_start)
    loss = 1.0 * lr_loss + l2_loss
    loss.backward()
    names, stats = [], []
    for k, p_ in unet.named_parameters():
        g = torch.zeros_like(p_) if p_.grad is None else p_.grad
        names.append(k)
        stats.append([g.double().sum().item(), g.double().norm().item()])
    cnames, cnorms = [], []
    for pre, m in (("cond_stage_model_1.", ld.cond_stage_model_1), ("cond_stage_model_2.", ld.cond_stage_model_2)):
        for k, p_ in m.named_parameters():
            cnames.append(pre + k)
            cnorms.append(0.0 if p_.grad is None else p_.grad.double().norm().item())
    frac = (x.detach().abs() >= 1.0).float().mean().item()
    print(f"loss {loss.item():.6f} = lr {lr_loss.item():.6f} + l2 {l2_loss.item():.6f}; clamped pixels {frac:.3f}; "
          f"|d c12| max {c12.grad.abs().max().item():.3e}")
    save("g18_tune.npz", t=t, timesteps=sm.ddim_timesteps, q_noise=q_noise, ddim_noise=torch.stack(draws),
         x_noisy=x_noisy.detach(), z=x_recon.detach(), image=decoded.detach().half(),
         loss=loss.detach(), lr_loss=lr_loss.detach(), l2_loss=l2_loss.detach(), dc12=c12.grad,
         names=np.asarray(names), stats=np.asarray(stats, dtype=np.float64),
         cond_names=np.asarray(cnames), cond_norms=np.asarray(cnorms, dtype=np.float64))
    torch.set_grad_enabled(False)


if __name__ == "__main__":
    gen_tune()
