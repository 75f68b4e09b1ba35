"""Generate tests/golden/g26_classifier.npz from the REAL face-reenactment reference (container only, CPU).

Usage (from the repository root):   python tools/make_golden_classifier.py

The reference's `NoisyLatentImageClassifier.shared_step` cannot run on the reference's own diffusion models (`get_x_noisy` reads
`diffusion_model.use_continuous_noise` and passes `continuous_sqrt_alpha_cumprod=` to `q_sample`; no model of the reference has
either, classifier.py:110-118), so this tool runs the three things `shared_step` is made of, in its order, from the reference's own
code: `DDPM.q_sample` (ddpm.py:273-276, on the reference's `make_beta_schedule` tables), `EncoderUNetModel` (openaimodel.py:745-961)
and `F.cross_entropy(reduction='none')`, then autograd.

Model: the reduced torso of g9 (`TRAIN_UNET`: model_channels 64, channel_mult [1, 2], one ResBlock per level, attention at both
levels, heads of 32) at image_size 16, 3 input channels, K = 8 classes -- an 8x8 final grid, 65 tokens in the attention pool, 448
pooled features -- built from the FR UNet's kwargs (use_spatial_transformer, context_dim, transformer_depth included: the encoder
swallows them), recipe weights (zero_module would make `adaptive`'s logits and every proj_out zero).  n = 3, t = (17, 803, 17),
y = (1, 7, 1).  Cases: the four pools in the legacy attention order, and `attention` with use_new_attention_order (`attention_new`).

Stored per case, under the prefix `<case>_`: logits, loss_per (reduction='none'), loss (their mean), names / shapes (the state
dict), stats ((sum, L2) of every parameter gradient of the mean loss), `grad:<key>` for the head's parameters and a handful of
torso parameters in full -- a tensor of more than 2048 elements as `gradpart:<key>`: rows [0, 8) x columns [0, 128) of its packed
[in][out] form (weight.reshape(out, -1).t()) -- dx (the gradient of the mean loss w.r.t. x_noisy), logp_grad (the gradient of
sum_b log p(y_b | x_b, t_b) w.r.t. x_noisy), `after:<key>` / `afterpart:<key>` (the same parameters after one
torch.optim.AdamW(lr=1e-4, weight_decay=1e-2) step).  Everything again with the whole reference in float64 (suffix `_f64`).  Only recorded arrays and name lists are stored.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import weights as W  # noqa: E402
from tools.make_golden import TRAIN_UNET, load_recipe, rnd, save  # noqa: E402

N, HW, K, T_IDX, LABELS, LR, WD = 3, 16, 8, (17, 803, 17), (1, 7, 1), 1e-4, 1e-2
SEEDS = dict(x0=261, noise=262)
CASES = dict(adaptive=dict(pool="adaptive"), attention=dict(pool="attention"), spatial=dict(pool="spatial"),
             spatial_v2=dict(pool="spatial_v2"), attention_new=dict(pool="attention", use_new_attention_order=True))
CLS_FULL_KEYS = ("time_embed.0.bias", "input_blocks.0.0.bias", "input_blocks.1.1.norm.weight", "input_blocks.2.0.op.bias",
                 "middle_block.0.in_layers.0.weight", "middle_block.1.proj_out.bias")
FULL_MAX = 2048


def packed_part(t):
    return t.reshape(t.shape[0], -1).t()[:8, :128]


def store(g, kind, key, name, t):
    t = t.detach()
    if t.numel() <= FULL_MAX:
        g[key(f"{kind}:{name}")] = t.float()
    else:
        g[key(f"{kind}part:{name}")] = packed_part(t).float()


def run_case(om, DDPM, make_beta_schedule, tag, settings, suffix, g, dt):
    cfg = dict(TRAIN_UNET, image_size=HW, in_channels=3, out_channels=K, **settings)
    model = om.EncoderUNetModel(**cfg)
    load_recipe(model, seed=0)
    model.train()
    if dt == torch.float64:
        model.double()
        model.dtype = torch.float64
        model.time_embed.register_forward_pre_hook(lambda mod, args: (args[0].double(),))
    # the schedule tables as DDPM.register_schedule makes them (float32 values in both runs, as the fp32 run has them)
    betas = make_beta_schedule("linear", W.SCHEDULE["timesteps"], linear_start=W.SCHEDULE["linear_start"],
                               linear_end=W.SCHEDULE["linear_end"], cosine_s=8e-3)
    ac = np.cumprod(1. - betas, axis=0)
    sched = types.SimpleNamespace(sqrt_alphas_cumprod=torch.tensor(np.sqrt(ac), dtype=torch.float32).to(dt),
                                  sqrt_one_minus_alphas_cumprod=torch.tensor(np.sqrt(1. - ac), dtype=torch.float32).to(dt))
    x0, noise = rnd(SEEDS["x0"], N, 3, HW, HW).to(dt), rnd(SEEDS["noise"], N, 3, HW, HW).to(dt)
    t, y = torch.tensor(T_IDX), torch.tensor(LABELS)
    key = lambda k: f"{tag}_{k}{suffix}"
    with torch.enable_grad():
        x_noisy = DDPM.q_sample(sched, x_start=x0, t=t, noise=noise).detach().requires_grad_(True)
        # (two forward passes: the reference's checkpoint function takes one backward pass per forward)
        logp = F.log_softmax(model(x_noisy, t), dim=-1)[torch.arange(N), y].sum()
        g[key("logp_grad")] = torch.autograd.grad(logp, x_noisy)[0].float()
        model.zero_grad(set_to_none=True)
        logits = model(x_noisy, t)
        per = F.cross_entropy(logits, y, reduction="none")
        loss = per.mean()
        loss.backward()
    g[key("logits")], g[key("loss_per")], g[key("loss")] = logits.detach().float(), per.detach().float(), loss.detach().float()
    g[key("dx")] = x_noisy.grad.float()
    names, shapes, stats = [], [], []
    for k, p_ in model.named_parameters():
        gr = torch.zeros_like(p_) if p_.grad is None else p_.grad
        names.append(k)
        shapes.append(",".join(str(s) for s in p_.shape))
        stats.append([gr.double().sum().item(), gr.double().norm().item()])
        if k.startswith("out.") or k in CLS_FULL_KEYS:
            store(g, "grad", key, k, gr)
    g[f"{tag}_names"], g[f"{tag}_shapes"] = np.asarray(names), np.asarray(shapes)
    g[key("stats")] = np.asarray(stats, dtype=np.float64)
    assert model._feature_size == 448 and logits.shape == (N, K)
    assert all(s[1] > 0 for s in stats), [n for n, s in zip(names, stats) if s[1] == 0]
    torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD).step()
    for k, p_ in model.named_parameters():
        if k.startswith("out.") or k in CLS_FULL_KEYS:
            store(g, "after", key, k, p_)
    print(f"  ({tag}{suffix}) loss {loss.item():.7g}  logits max {logits.abs().max().item():.4g}  |dx| {x_noisy.grad.norm().item():.4g}")


def gen_classifier():
    from tools import ref_shims
    ref_shims.install("face_reenactment")
    from ldm.models.diffusion.ddpm import DDPM
    from ldm.modules.diffusionmodules import openaimodel as om
    from ldm.modules.diffusionmodules.util import GroupNorm32, make_beta_schedule
    g = {}
    print("[G26] fp32 reference")
    for tag, settings in CASES.items():
        run_case(om, DDPM, make_beta_schedule, tag, settings, "", g, torch.float32)
    print("[G26] the whole reference in float64")
    gn32 = GroupNorm32.forward
    GroupNorm32.forward = torch.nn.GroupNorm.forward         # the float32 pin of the reference, lifted in memory only
    try:
        for tag, settings in CASES.items():
            torch.set_default_dtype(torch.float32)
            run_case(om, DDPM, make_beta_schedule, tag, settings, "_f64", g, torch.float64)
    finally:
        torch.set_default_dtype(torch.float32)
        GroupNorm32.forward = gn32
    for k in sorted(g):
        if k.endswith("_f64") and k[:-4] in g and "stats" not in k:
            a, b = torch.as_tensor(g[k[:-4]]).double(), torch.as_tensor(g[k]).double()
            print(f"  {k[:-4]:56s} max|fp32 - f64| {(a - b).abs().max().item():.3e}  max|f64| {b.abs().max().item():.4g}")
    for k, v in g.items():
        if k.endswith("names") or k.endswith("shapes"):
            continue
        assert torch.isfinite(torch.as_tensor(v).double()).all(), k
    save("g26_classifier.npz", **g)


if __name__ == "__main__":
    gen_classifier()
