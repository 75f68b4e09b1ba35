"""Generate tests/golden/g25_objective.npz from the REAL face-reenactment reference (container only, CPU).

Usage (from the repository root):   python tools/make_golden_objective.py

The reference's own `LatentDiffusion.p_losses` (ddpm.py:1014-1047) + autograd on the reduced training UNet of g9 (`TRAIN_UNET`,
recipe weights, seeded inputs), for the two settings of the objective the default fixture does not reach, n = 3 at 16x16 with
t = (17, 803, 17) -- two samples share a timestep, so the dense logvar gradient has to add them:
  (a) eps, l1, l_simple_weight 0.8, original_elbo_weight 10, learn_logvar, logvar_init -0.7
  (b) x0,  l2, original_elbo_weight 1, logvar_init 0.3 (fixed)
Stored like g9, under the prefixes `a_` / `b_`: (sum, L2) of every parameter gradient, the TRAIN_FULL_KEYS gradients in full,
dcontext, every entry of the loss dictionary, lvlb_weights; for (a) the logvar gradient and logvar after one
torch.optim.AdamW(lr=1e-4) step; for (b) p_sample_loop(timesteps=3) with its pinned draws.  Everything is repeated with the whole
reference in float64 (suffix `_f64`).  Only recorded arrays are stored.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import weights as W  # noqa: E402
from tools.make_golden import TRAIN_FULL_KEYS, TRAIN_UNET, load_recipe, rnd, save  # noqa: E402

N, HW, T_IDX, LR = 3, 16, (17, 803, 17), 1e-4
CASES = dict(
    a=dict(parameterization="eps", loss_type="l1", l_simple_weight=0.8, original_elbo_weight=10., learn_logvar=True, logvar_init=-0.7),
    b=dict(parameterization="x0", loss_type="l2", original_elbo_weight=1., logvar_init=0.3))
SEEDS = dict(x0=101, noise=102, ctx=103, xT=254, draws=25)


def build(LatentDiffusion, settings):
    unet_cfg = dict(target="ldm.modules.diffusionmodules.openaimodel.UNetModel", params=dict(TRAIN_UNET))
    fs_cfg = dict(target="ldm.models.autoencoder.VQModelInterface",
                  params=dict(embed_dim=3, n_embed=16384, ddconfig=dict(W.VQ_F4["ddconfig"]),
                              lossconfig=dict(target="torch.nn.Identity")))
    cond_cfg = dict(target="ldm.modules.encoders.modules.ClassEmbedder3",
                    params=dict(embed_dim=512, n_classes=8, key="class_label", p_uncond=0.2))
    ld = LatentDiffusion(first_stage_config=fs_cfg, cond_stage_config=cond_cfg, num_timesteps_cond=1,
                         cond_stage_key="class_label", cond_stage_trainable=True, conditioning_key="crossattn",
                         unet_config=unet_cfg, image_size=HW, channels=3, first_stage_key="image", log_every_t=200,
                         monitor="val_loss_ema", **W.SCHEDULE, **settings)
    load_recipe(ld.model.diffusion_model, seed=0, prefix_check=W.unet_param_shapes(TRAIN_UNET))
    return ld


def run_case(ld, tag, suffix, g, dt):
    """One p_losses + backward (+ the AdamW step of a learned logvar, + the ancestral loop of an x0 model) -> entries of g."""
    unet = ld.model.diffusion_model
    ld.train()
    torch.set_grad_enabled(True)
    x0, noise = rnd(SEEDS["x0"], N, 3, HW, HW).to(dt), rnd(SEEDS["noise"], N, 3, HW, HW).to(dt)
    c = rnd(SEEDS["ctx"], N, 1, 512).to(dt).requires_grad_(True)
    t = torch.tensor(T_IDX)
    loss, loss_dict = ld.p_losses(x0, c, t, noise=noise)
    loss.backward()
    key = lambda k: f"{tag}_{k}{suffix}"
    g[key("loss")] = loss.detach().float()
    for k, v in loss_dict.items():
        g[key("dict:" + k)] = v.detach().float()
    g[key("dcontext")] = c.grad.float()
    names, stats = [], []
    for k, p_ in unet.named_parameters():
        gr = torch.zeros_like(p_) if p_.grad is None else p_.grad
        names.append(k)
        stats.append([gr.double().sum().item(), gr.double().norm().item()])
        if k in TRAIN_FULL_KEYS:
            g[key("grad:" + k)] = gr.float()
    g[f"{tag}_names"] = np.asarray(names)
    g[key("stats")] = np.asarray(stats, dtype=np.float64)
    g[key("lvlb_weights")] = ld.lvlb_weights.float()
    if ld.learn_logvar:
        dlv = ld.logvar.grad.detach().clone()
        off = torch.ones(dlv.shape[0], dtype=torch.bool)
        off[list(set(T_IDX))] = False
        assert (dlv[off] == 0).all() and (dlv[~off] != 0).all(), "dlogvar must be non-zero on the drawn timesteps and zero elsewhere"
        g[key("dlogvar")] = dlv.float()
        torch.optim.AdamW([ld.logvar], lr=LR).step()
        g[key("logvar_after")] = ld.logvar.detach().float()
        vlb = ld.original_elbo_weight * loss_dict["train_loss_vlb"].item() / loss.item()
        print(f"  ({tag}{suffix}) loss {loss.item():.6g}  loss_vlb {loss_dict['train_loss_vlb'].item():.6g}  VLB share {100 * vlb:.1f} %  "
              f"dlogvar[17] {dlv[17].item():.6g}  dlogvar[803] {dlv[803].item():.6g}")
        assert 0.1 <= vlb <= 0.9, "the VLB term must carry 10-90 % of the loss, or the fixture does not test its weight"
    else:
        print(f"  ({tag}{suffix}) loss {loss.item():.6g}  loss_vlb {loss_dict['train_loss_vlb'].item():.6g}")
    torch.set_grad_enabled(False)
    if ld.parameterization == "x0":
        ld.eval()
        xT = rnd(SEEDS["xT"], N, 3, HW, HW).to(dt)
        # the float64 twin is fed the fp32 run's draws: a float64 randn gives other values from the same seed, so noise_like's
        # torch.randn draws in float32 and widens (patched in memory for the loop only)
        randn = torch.randn
        if suffix:
            torch.randn = lambda *a, **k: randn(*a, **dict(k, dtype=torch.float32)).to(dt)
        try:
            torch.manual_seed(SEEDS["draws"])
            out = ld.p_sample_loop(c.detach(), (N, 3, HW, HW), x_T=xT, timesteps=3, verbose=False)
        finally:
            torch.randn = randn
        torch.manual_seed(SEEDS["draws"])
        nz = torch.stack([torch.randn(xT.shape, dtype=torch.float32) for _ in range(3)])
        assert torch.isfinite(out).all() and out.dtype == dt
        g[key("p_sample_loop_T3")] = out.float()
        g[f"{tag}_p_sample_loop_noise"] = nz


def gen_objective():
    from tools import ref_shims
    ref_shims.install("face_reenactment")
    from ldm.models.diffusion.ddpm import LatentDiffusion
    from ldm.modules.diffusionmodules.util import GroupNorm32
    g = {}
    print("[G25] fp32 reference")
    for tag, settings in CASES.items():
        run_case(build(LatentDiffusion, settings), tag, "", g, torch.float32)
    print("[G25] the whole reference in float64")
    # the three float32 pins of the reference, lifted in memory only (tools/make_golden_plms.py does the same)
    gn32 = GroupNorm32.forward
    GroupNorm32.forward = torch.nn.GroupNorm.forward
    try:
        for tag, settings in CASES.items():
            torch.set_default_dtype(torch.float32)
            ld = build(LatentDiffusion, settings)         # (the schedule buffers are float32 values, as the fp32 run has them)
            torch.set_default_dtype(torch.float64)
            ld.double()
            unet = ld.model.diffusion_model
            unet.dtype = torch.float64
            unet.time_embed.register_forward_pre_hook(lambda mod, args: (args[0].double(),))
            run_case(ld, tag, "_f64", g, torch.float64)
    finally:
        torch.set_default_dtype(torch.float32)
        GroupNorm32.forward = gn32
    for k in sorted(g):
        if k.endswith("_f64") and k[:-4] in g and "stats" not in k:
            a, b = torch.as_tensor(g[k[:-4]]).double(), torch.as_tensor(g[k]).double()
            print(f"  {k[:-4]:48s} max|fp32 - f64| {(a - b).abs().max().item():.3e}  max|f64| {b.abs().max().item():.4g}")
    for k, v in g.items():
        if k.endswith("names"):
            continue
        assert torch.isfinite(torch.as_tensor(v).double()).all() or "lvlb" in k, k
    save("g25_objective.npz", **g)


if __name__ == "__main__":
    gen_objective()
