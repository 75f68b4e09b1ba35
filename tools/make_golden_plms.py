"""Generate tests/golden/g22_plms.npz, g22_plms_f64.npz and g22_plms_options.npz from the REAL face-reenactment reference (container only, CPU).

Usage (from the repository root):   python tools/make_golden_plms.py

`PLMSSampler` (ldm/models/diffusion/plms.py:11-236; the talking-face tree carries an identical copy) over the reference
`LatentDiffusion` with the recipe weights of `make_fr_model(gain=0.25)` and seeded inputs: B = 2 at the 32x32x3 latent, labels
[1, 6].  S = 5 is the smallest run that takes every branch of p_sample_plms: Euler, order 2, order 3, order 4 with a full list,
order 4 after the list has dropped its oldest entry.  The option cases run at S = 4: the reference's 'uniform' discretisation has no
S = 3 (1000 // 3 = 333 gives the four timesteps 1, 334, 667, 1000, and make_ddim_sampling_parameters indexes alphas_cumprod[1000]:
IndexError, util.py:65).  The plain runs are repeated with the whole reference in float64 (g22_plms_f64.npz); the distance
d = max |fp32 - float64| of each run is printed, and with it the bound max(1.5e-4, 4 d) the GPU tests hold that run's cases to.
Only recorded arrays are stored, float32, in three files that each stay well under the size limit for a committed file.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import weights as W  # noqa: E402
from tools.make_golden import ShiftCorrector, load_recipe, rnd, save  # noqa: E402
from tools.make_golden_split import SPLIT, H, W_  # noqa: E402


def gen_plms():
    from tools import ref_shims
    ref_shims.install("face_reenactment")
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.models.diffusion.plms import PLMSSampler
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

    class CPUPLMS(PLMSSampler):          # the reference hard-codes .to('cuda')
        def register_buffer(self, n, a):
            setattr(self, n, a)

    sampler = CPUPLMS(ld)
    labels = torch.tensor([1, 6])
    c = ld.cond_stage_model.embedding(labels[:, None])
    uc = ld.cond_stage_model.uncond_embedding(torch.zeros(2, 1, dtype=torch.long))
    xT = rnd(221, 2, 3, 32, 32)
    g, gopt, g64 = {}, {}, {}              # -> g22_plms.npz, g22_plms_options.npz, g22_plms_f64.npz
    S_OPT = 4
    kw = dict(batch_size=2, shape=[3, 32, 32], conditioning=c, eta=0.0, x_T=xT, verbose=False)
    cfg3 = dict(unconditional_guidance_scale=3.0, unconditional_conditioning=uc)

    def record(tag, out, inter):           # the whole lists (the sample is x_inter[-1])
        assert torch.equal(out, inter["x_inter"][-1])
        g[tag + "_x_inter"] = torch.stack(inter["x_inter"])
        g[tag + "_pred_x0"] = torch.stack(inter["pred_x0"])

    def record_last(tag, out, inter):      # option runs: the sample and the last pred_x0
        gopt[tag], gopt[tag + "_pred_x0"] = out, inter["pred_x0"][-1]

    print("[G22] PLMSSampler.sample S=5, guidance 1 and 3, log_every_t=1")
    record("sample_S5", *sampler.sample(S=5, log_every_t=1, **kw))
    record("sample_S5_cfg", *sampler.sample(S=5, log_every_t=1, **kw, **cfg3))
    assert g["sample_S5_x_inter"].shape[0] == 6            # x_T and one entry per step

    print("[G22] p_sample_plms with 0..3 past outputs")
    sampler.make_schedule(ddim_num_steps=5, ddim_eta=0.0, verbose=False)
    g["ddim_timesteps_S5"] = np.asarray(sampler.ddim_timesteps)
    x = rnd(222, 2, 3, 32, 32)
    old = [0.9 * rnd(223 + j, 2, 3, 32, 32) for j in range(3)]                  # oldest first, as the loop appends them
    # (the inputs are regenerated from their seeds by the tests)
    index = 3
    t = torch.full((2,), int(sampler.ddim_timesteps[index]), dtype=torch.long)
    t_next = torch.full((2,), int(sampler.ddim_timesteps[index - 1]), dtype=torch.long)
    for k in range(4):
        outs = sampler.p_sample_plms(x, c, t, index=index, old_eps=old[3 - k:], t_next=t_next, **cfg3)
        gopt[f"p_sample_n{k}"] = torch.stack(outs)            # (x_prev, pred_x0, e_t)

    print("[G22] timesteps=3 subset at S=5")
    out, inter = sampler.plms_sampling(c, (2, 3, 32, 32), x_T=xT, timesteps=3, log_every_t=1)
    record("subset_S5_t3", out, inter)
    print(f"  {g['subset_S5_t3_x_inter'].shape[0] - 1} steps")

    print(f"[G22] plain runs at S={S_OPT} (the float64 twins of these give the option cases their bound)")
    record_last("sample_S4", *sampler.sample(S=S_OPT, log_every_t=1, **kw))
    record_last("sample_S4_cfg", *sampler.sample(S=S_OPT, log_every_t=1, **kw, **cfg3))

    print(f"[G22] quantize_x0, S={S_OPT}")
    record_last("quantize_S4", *sampler.sample(S=S_OPT, log_every_t=1, quantize_x0=True, **kw))

    print(f"[G22] mask + x0, S={S_OPT}, guidance 3")
    # the reference draws, per step, q_sample's randn_like and then noise_like's randn once per get_x_prev_and_pred_x0 call --
    # twice in step 0 (plms.py:221,234).  sigma is 0, so only q_sample's draws reach the result: they are replayed and stored.
    x0, mask = 0.5 * rnd(226, 2, 3, 32, 32), (rnd(227, 2, 1, 32, 32) > 0).float()
    torch.manual_seed(22)
    mz = []
    for i in range(S_OPT):
        mz.append(torch.randn(xT.shape))
        for _ in range(2 if i == 0 else 1):
            torch.randn(xT.shape)
    torch.manual_seed(22)
    out, inter = sampler.sample(S=S_OPT, log_every_t=1, mask=mask, x0=x0, **kw, **cfg3)
    record_last("mask_S4_cfg", out, inter)
    gopt["mask_noise"] = torch.stack(mz)
    # the replay is right iff the run is reproduced by a loop that injects it (checked on the first blend: x_inter[1] depends on mz[0])
    a = ld.sqrt_alphas_cumprod[int(np.flip(sampler.ddim_timesteps)[0])]
    s = ld.sqrt_one_minus_alphas_cumprod[int(np.flip(sampler.ddim_timesteps)[0])]
    blended = (a * x0 + s * mz[0]) * mask + (1. - mask) * xT
    last = S_OPT - 1
    outs = sampler.p_sample_plms(blended, c, torch.full((2,), int(sampler.ddim_timesteps[last]), dtype=torch.long), index=last, old_eps=[],
                                 t_next=torch.full((2,), int(sampler.ddim_timesteps[last - 1]), dtype=torch.long), **cfg3)
    torch.testing.assert_close(outs[0], inter["x_inter"][1], rtol=0, atol=0)

    print(f"[G22] score_corrector, S={S_OPT}, guidance 3")
    record_last("corrector_S4_cfg", *sampler.sample(S=S_OPT, log_every_t=1, score_corrector=ShiftCorrector(), corrector_kwargs=dict(strength=0.2),
                                               **kw, **cfg3))

    print(f"[G22] patch-wise, 48x64 latent, S={S_OPT}")
    ld.split_input_params = dict(SPLIT)
    xTs = rnd(228, 2, 3, H, W_)
    gopt["split_S4"], _ = sampler.sample(S=S_OPT, batch_size=2, shape=[3, H, W_], conditioning=c, eta=0.0, x_T=xTs, verbose=False)
    del ld.split_input_params

    print("[G22] the plain runs with the whole reference in float64")
    # the reference pins float32 in three places, lifted here in memory only: UNetModel.dtype (`x.type(self.dtype)`), GroupNorm32
    # (`x.float()`), and timestep_embedding, whose float32 sinusoid is widened on its way into time_embed (both runs then see the
    # same embedding values, so its rounding is not part of d: d can only come out smaller, and the bound tighter, for that)
    from ldm.modules.diffusionmodules.util import GroupNorm32
    ld.double()
    unet = ld.model.diffusion_model
    unet.dtype = torch.float64
    GroupNorm32.forward = torch.nn.GroupNorm.forward
    unet.time_embed.register_forward_pre_hook(lambda mod, args: (args[0].double(),))
    kw64 =dict(kw, conditioning=c.double(), x_T=xT.double())
    cfg64 = dict(unconditional_guidance_scale=3.0, unconditional_conditioning=uc.double())
    torch.set_default_dtype(torch.float64)                 # timestep_embedding, torch.full(...) and friends follow the default
    try:
        s64 = CPUPLMS(ld)
        o64 = {"sample_S5": s64.sample(S=5, log_every_t=1, **kw64), "sample_S5_cfg": s64.sample(S=5, log_every_t=1, **kw64, **cfg64),
               "sample_S4": s64.sample(S=S_OPT, log_every_t=1, **kw64), "sample_S4_cfg": s64.sample(S=S_OPT, log_every_t=1, **kw64, **cfg64)}
    finally:
        torch.set_default_dtype(torch.float32)
    for tag, (out, inter) in o64.items():
        assert out.dtype == torch.float64
        if tag.startswith("sample_S5"):
            pairs = {tag + "_x_inter": torch.stack(inter["x_inter"]), tag + "_pred_x0": torch.stack(inter["pred_x0"])}
            ref32 = g
        else:
            pairs = {tag: out, tag + "_pred_x0": inter["pred_x0"][-1]}
            ref32 = gopt
        d = 0.0
        for k, v in pairs.items():
            g64[k + "_f64"] = v.float()
            d = max(d, (g64[k + "_f64"] - torch.as_tensor(ref32[k])).abs().max().item())      # from the arrays as stored
        print(f"  {tag:14s} d = max |fp32 reference - float64 reference| = {d:.3e} (|x| up to {out.abs().max().item():.2f});  "
              f"bound max(1.5e-4, 4 d) = {max(1.5e-4, 4 * d):.3e}")

    for name, gg in (("g22_plms.npz", g), ("g22_plms_options.npz", gopt), ("g22_plms_f64.npz", g64)):
        for k, v in gg.items():
            v = torch.as_tensor(v)
            assert torch.isfinite(v.double()).all(), k
            print(f"  {k:26s} {tuple(v.shape)}  max|.| {v.double().abs().max().item():.4g}")
        save(name, **gg)


if __name__ == "__main__":
    gen_plms()
