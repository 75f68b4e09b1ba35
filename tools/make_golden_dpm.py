"""Generate tests/golden/g23_dpm.npz, g23_dpm_options.npz and g23_dpm_f64.npz from the REAL reference (container only, CPU).

Usage (from the repository root):   python tools/make_golden_dpm.py

The solver is the talking-face tree's `ldm/models/diffusion/dpm_solver/dpm_solver.py` (it imports torch and math only, so it is
loaded by path), driven the way that tree's `DPMSolverSampler.sample` drives it (sampler.py:67-80: NoiseScheduleVP('discrete'),
model_wrapper(..., 'noise', 'classifier-free'), DPM_Solver(predict_x0=True, thresholding=False).sample(method='multistep')) --
the sampler class itself hard-codes .to('cuda').  The model is the PLMS fixtures' (tools/make_golden_plms.py): the reference
`LatentDiffusion` with the recipe weights of `make_fr_model(gain=0.25)`, B = 2 at the 32x32x3 latent, labels [1, 6].

Recorded per run: the latent and the model time `t_input` of every model evaluation plus the final latent (`x_inter`), and the
schedule scalars as the reference formed them -- time steps, lambda, and every coefficient on its way through `expand_dims`, laid
out like the rows of `dsml_thesis_amd.dpm_solver.step_table`.  Every run is repeated with the whole reference in float64; the
distance d = max |fp32 - float64| over ALL of a run's latents is stored with the twin (`<tag>_d`) and printed with the bound
max(1.5e-4, 4 d) the GPU tests hold that run to.  The twins of the two S = 5 runs are stored whole, the others by their final
latent; each file stays under the size limit for a committed file.

The order-3 run has lower_order_final=False (orders 1, 2, 3, 3, 3, 3).  With lower_order_final the reference cannot run order 3 in
fewer than 15 steps: when the order drops to 2 it hands the three-entry history to multistep_dpm_solver_second_update, which
unpacks two (`model_prev_1, model_prev_0 = model_prev_list`, dpm_solver.py:773: ValueError).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import weights as W  # noqa: E402
from tools.make_golden import load_recipe, rnd, save  # noqa: E402
from tools.make_golden_split import SPLIT, H, W_  # noqa: E402

SOLVER = ("talking_face", "ldm", "models", "diffusion", "dpm_solver", "dpm_solver.py")      # under the reference's root
N_COEF = {1: 2, 2: 4, 3: 8}          # expand_dims calls of one multistep update, by order

# tag -> (S, keywords of DPM_Solver.sample, guidance, which x_inter entries are stored (None: all))
RUNS = {
    "S5": (5, dict(order=2), 1., None),
    "S5_cfg": (5, dict(order=2), 3., None),
    "S6_o3": (6, dict(order=3, lower_order_final=False), 1., None),
    "S2": (2, dict(order=2), 1., None),
}
OPTION_RUNS = {
    "S15": (15, dict(order=2), 1., list(range(0, 16, 3))),
    "S5_logSNR": (5, dict(order=2, skip_type="logSNR"), 1., None),
    "S5_quadratic": (5, dict(order=2, skip_type="time_quadratic"), 1., None),
    "S5_nolof": (5, dict(order=2, lower_order_final=False), 1., None),
}


def gen_dpm():
    from tools import ref_shims
    ref_shims.install("face_reenactment")
    import ldm
    from ldm.models.diffusion.ddpm import LatentDiffusion
    ref_root = os.path.dirname(os.path.dirname(os.path.abspath(list(ldm.__path__)[0])))     # the two trees' parent
    spec = importlib.util.spec_from_file_location("ref_dpm_solver", os.path.join(ref_root, *SOLVER))
    D = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(D)
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

    labels = torch.tensor([1, 6])
    c = ld.cond_stage_model.embedding(labels[:, None])
    uc = ld.cond_stage_model.uncond_embedding(torch.zeros(2, 1, dtype=torch.long))
    xT = rnd(231, 2, 3, 32, 32)
    xTs = rnd(232, 2, 3, H, W_)

    seen = []                                              # every vector that passes through expand_dims, in order
    plain_expand = D.expand_dims

    def recording_expand(v, dims):
        seen.append(v.reshape(-1)[0].clone())
        return plain_expand(v, dims)
    D.expand_dims = recording_expand

    def run(S, kw, scale, x_start, dtype=torch.float32):
        """-> (x_inter [S + 1], t_input [S], scalars dict); the reference's own calls, sampler.py:67-80."""
        ns = D.NoiseScheduleVP("discrete", alphas_cumprod=ld.alphas_cumprod.clone().detach().to(dtype))
        xs, tin = [], []

        def apply(x, t, cc):
            b = x_start.shape[0]
            xs.append(x[:b].clone())
            tin.append(t[0].clone())
            return ld.apply_model(x, t, cc)
        model_fn = D.model_wrapper(apply, ns, model_type="noise", guidance_type="classifier-free", condition=c.to(dtype),
                                   unconditional_condition=uc.to(dtype), guidance_scale=scale)
        solver = D.DPM_Solver(model_fn, ns, predict_x0=True, thresholding=False)
        del seen[:]
        args = dict(dict(skip_type="time_uniform", method="multistep", order=2, lower_order_final=True), **kw)
        out = solver.sample(x_start.to(dtype), steps=S, **args)
        assert len(xs) == S
        ts = solver.get_time_steps(args["skip_type"], ns.T, 1. / ns.total_N, S, "cpu")
        lam = torch.cat([ns.marginal_lambda(ts[k].expand(2))[:1] for k in range(S + 1)])
        # the expand_dims stream: per step [sigma_s, alpha_s] of the model evaluation, then the update's coefficients
        orders = list(range(1, args["order"]))
        for step in range(args["order"], S + 1):
            orders.append(min(args["order"], S + 1 - step) if (args["lower_order_final"] and S < 15) else args["order"])
        coef = torch.zeros(S, 12, dtype=dtype)
        flat = list(seen)
        for k, o in enumerate(orders):
            sig_s, al_s = flat[:2]
            u = flat[2:2 + N_COEF[o]]
            flat = flat[2 + N_COEF[o]:]
            coef[k, 0], coef[k, 1], coef[k, 2] = al_s, sig_s, float(o)
            if o == 1:
                coef[k, 3], coef[k, 4] = u
            elif o == 2:
                coef[k, 5], coef[k, 3], coef[k, 4] = u[0], u[1], u[2]
                assert torch.equal(u[2], u[3])
            else:
                coef[k, 5], coef[k, 6], coef[k, 7], coef[k, 8], coef[k, 3], coef[k, 4], coef[k, 9], coef[k, 10] = u
        assert not flat, len(flat)
        sc = dict(timesteps=ts, lam=lam, coef=coef, orders=np.asarray(orders), t_input=torch.stack(tin))
        return xs + [out], sc

    g, gopt, g64 = {}, {}, {}

    def record(dst, tag, S, kw, scale, keep, x_start=xT):
        print(f"[G23] {tag}: S={S} {kw} guidance {scale}", flush=True)
        xi, sc = run(S, kw, scale, x_start)
        for k, v in sc.items():
            dst[f"{tag}_{k}"] = v
        idx = list(range(S + 1)) if keep is None else keep
        dst[f"{tag}_x_inter"] = torch.stack([xi[i] for i in idx])
        dst[f"{tag}_x_inter_idx"] = np.asarray(idx)
        return xi

    full = {}
    for tag, (S, kw, scale, keep) in RUNS.items():
        full[tag] = record(g, tag, S, kw, scale, keep)
    for tag, (S, kw, scale, keep) in OPTION_RUNS.items():
        full[tag] = record(gopt, tag, S, kw, scale, keep)
    ld.split_input_params = dict(SPLIT)
    full["split_S5"] = record(gopt, "split_S5", 5, dict(order=2), 1., [1, 5], x_start=xTs)
    del ld.split_input_params

    print("[G23] every run again with the whole reference in float64", flush=True)
    # the reference pins float32 in three places, lifted here in memory only (tools/make_golden_plms.py): UNetModel.dtype,
    # GroupNorm32, and timestep_embedding, whose float32 sinusoid (of the float32-rounded model time) is widened on its way into
    # time_embed.  The float64 solver's own scalars and model times differ from the float32 ones by their rounding: part of d.
    from ldm.modules.diffusionmodules.util import GroupNorm32
    ld.double()
    unet = ld.model.diffusion_model
    unet.dtype = torch.float64
    GroupNorm32.forward = torch.nn.GroupNorm.forward
    unet.time_embed.register_forward_pre_hook(lambda mod, args: (args[0].double(),))
    torch.set_default_dtype(torch.float64)
    try:
        twins = {}
        for tag, (S, kw, scale, _) in list(RUNS.items()) + list(OPTION_RUNS.items()):
            print(f"  {tag}", flush=True)
            twins[tag] = run(S, kw, scale, xT, torch.float64)[0]
        ld.split_input_params = dict(SPLIT)
        print("  split_S5", flush=True)
        twins["split_S5"] = run(5, dict(order=2), 1., xTs, torch.float64)[0]
        del ld.split_input_params
    finally:
        torch.set_default_dtype(torch.float32)
    for tag, xi64 in twins.items():
        assert xi64[-1].dtype == torch.float64
        x64 = torch.stack(xi64).float()
        x32 = torch.stack(full[tag])
        d = (x64 - x32).abs().max().item()
        g64[f"{tag}_d"] = np.float32(d)
        g64[f"{tag}_final_f64"] = x64[-1]
        if tag in ("S5", "S5_cfg"):
            g64[f"{tag}_x_inter_f64"] = x64
        print(f"  {tag:14s} d = max |fp32 reference - float64 reference| = {d:.3e} (|x| up to {x32.abs().max().item():.2f});  "
              f"bound max(1.5e-4, 4 d) = {max(1.5e-4, 4 * d):.3e}")

    for name, gg in (("g23_dpm.npz", g), ("g23_dpm_options.npz", gopt), ("g23_dpm_f64.npz", g64)):
        for k, v in gg.items():
            v = torch.as_tensor(v)
            assert torch.isfinite(v.double()).all(), k
            print(f"  {k:26s} {tuple(v.shape)}  max|.| {v.double().abs().max().item():.4g}")
        save(name, **gg)


if __name__ == "__main__":
    gen_dpm()
