"""Generate tests/golden/g27_dpm_methods_*.npz and g27_dpm_methods_f64.npz from the REAL reference (container only, CPU).

Usage (from the repository root):   python tools/make_golden_dpm_methods.py

The solver is the talking-face tree's `ldm/models/diffusion/dpm_solver/dpm_solver.py`, loaded by path as tools/make_golden_dpm.py
loads it, and driven through its own public surface: NoiseScheduleVP('discrete'), model_wrapper(..., 'noise', 'classifier-free'),
DPM_Solver(model_fn, ns, predict_x0, thresholding, max_val).sample(...).  Model, labels and start noise are those of
tools/make_golden_dpm.py (the recipe weights of `make_fr_model(gain=0.25)`, B = 2 at 32x32x3, labels [1, 6], x_T = rnd(231, ...)).

Recorded per run: the latent entering every model evaluation plus the final one (`x_inter`), the model time of every evaluation
(`t_input`), the outer time steps and orders, r1 / r2 of every singlestep outer step as `sample` handed them on, and the
coefficients as the reference formed them on their way through `expand_dims`, laid out like the rows of
`dsml_thesis_amd.dpm_solver.method_table` (`coef`; the reference's Python-float and 0-dim factors (0.5 / r1), r2 / r1, (1. / r2) and
its sign are applied here to the recorded scalars, in the reference's order).  Thresholded runs also store `s` per evaluation and
sample, and `max_val`.  Every run is repeated with the whole reference in float64; d = max |fp32 - float64| over ALL of a run's
latents is stored with the twin's final latent (`<tag>_d`, `<tag>_final_f64`).

Asserted here (a run that breaks one gets other settings, the rule stays):
  (a) across the thresholded runs some (evaluation, sample) has s > max_val and some has s == max_val.  `max_val` of the run tagged
      thr_ms2_5 is taken from a probe run at max_val = 1 (the median of its raw quantiles, two significant digits);
  (b) in every thresholded run clamping changes at least one element;
  (c) max(1.5e-4, 4 d) <= 2^-15 max |latent| for every run whose latents can reach 1.5e-4 * 2^15 = 4.9 at all.  The thresholded runs
      cannot (x0 is clamped into [-1, 1], so |latent| stays near |x_T|max = 3.71 and the floor 1.5e-4 alone is 2^-14.6 of it, whatever
      the steps or the guidance scale); they are held to 4 d <= 1.5e-4, i.e. the floor is their whole bound.
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
from tools.make_golden_dpm import SOLVER  # noqa: E402
from tools.make_golden_split import SPLIT, H, W_  # noqa: E402

ROW = 16
N_MS = {1: 2, 2: 4, 3: 8}            # expand_dims calls of one multistep update, by order
FILE_BYTES = 880 * 1024              # raw float32 bytes of x_inter per fixture file (each file stays under 1 MiB)

# tag -> (keywords of DPM_Solver(...), keywords of .sample(...), guidance scale)
X0 = dict(predict_x0=True)
RUNS = {
    "ss3_6": (X0, dict(steps=6, order=3), 1.),
    "ss3_4": (X0, dict(steps=4, order=3), 1.),
    "ss3_5": (X0, dict(steps=5, order=3), 1.),
    "ss2_5": (X0, dict(steps=5, order=2), 1.),
    "ssf2_6": (X0, dict(steps=6, order=2, method="singlestep_fixed"), 1.),
    "ss3_6_logSNR": (X0, dict(steps=6, order=3, skip_type="logSNR"), 1.),
    "ss2_4_quadratic": (X0, dict(steps=4, order=2, skip_type="time_quadratic"), 1.),
    "eps_ss3_6": ({}, dict(steps=6, order=3), 1.),
    "eps_ms2_5": ({}, dict(steps=5, order=2, method="multistep"), 1.),
    "eps_ms3_6": ({}, dict(steps=6, order=3, method="multistep", lower_order_final=False), 1.),
    "tay_ss3_6": (X0, dict(steps=6, order=3, solver_type="taylor"), 1.),
    "tay_ss2_4": (X0, dict(steps=4, order=2, solver_type="taylor"), 1.),
    "tay_ms2_5": (X0, dict(steps=5, order=2, method="multistep", solver_type="taylor"), 1.),
    "eps_tay_ss3_6": ({}, dict(steps=6, order=3, solver_type="taylor"), 1.),
    "cfg_ss3_6": (X0, dict(steps=6, order=3), 3.),
    "thr_ms2_5": (dict(predict_x0=True, thresholding=True), dict(steps=5, order=2, method="multistep"), 1.),      # max_val: see (a)
    "thr_cfg_ss3_6": (dict(predict_x0=True, thresholding=True), dict(steps=6, order=3), 3.),
    "dz_ms2_5": (X0, dict(steps=5, order=2, method="multistep", denoise_to_zero=True), 1.),
    "sub_ss2_4": (X0, dict(steps=4, order=2, t_start=0.6, t_end=0.1), 1.),
    "split_ss2_4": (X0, dict(steps=4, order=2), 1.),
}
PROBED = "thr_ms2_5"


def fold(stream, rs, method, orders, x0, taylor, thr, thr_denoise, denoise, dtype):
    """The expand_dims stream of one run -> [n_eval][ROW] in method_table's layout (column 15, the next model time, and the flags
    are left 0: t_input is stored on its own).  rs: (r1, r2) per singlestep outer step, 0-dim tensors as `sample` formed them."""
    it = iter(stream)
    take = lambda n: [next(it) for _ in range(n)]
    rows = []
    sign = (lambda v: v) if x0 else (lambda v: -v)

    def evaluation(form_x0, thresholded):                  # data_prediction_fn: sigma_t, alpha_t[, s] (:393-397)
        row = torch.zeros(ROW, dtype=dtype)
        if form_x0:
            row[1], row[0] = take(2)
            if thresholded:
                take(1)
        rows.append(row)
        return row

    if method == "multistep":
        for k, o in enumerate(orders):
            row = evaluation(x0, thr)
            u = take(N_MS[o])
            if o == 1:
                row[2], row[3], row[4] = 4., u[0], u[1]
            elif o == 2:
                row[2], row[5], row[3], row[4] = 5., u[0], u[1], u[2]
                row[9] = sign(u[3]) if taylor else -(0.5 * u[3])
                assert taylor or torch.equal(u[2], u[3])
            else:
                row[2], row[5], row[6], row[7], row[8], row[3], row[4], row[9], row[10] = 6., u[0], u[1], u[2], u[3], u[4], u[5], sign(u[6]), u[7]
    else:
        for o, (r1, r2) in zip(orders, rs):
            row = evaluation(x0, thr)
            row[2], row[3], row[4] = [0.] + take(2)
            if o == 1:
                continue
            row = evaluation(x0, thr)
            cx, c0, third = take(3)
            row[3], row[4] = cx, c0
            if o == 2:
                row[2] = 2.
                row[5] = sign((1. / r1) * third) if taylor else -((0.5 / r1) * third)
                continue
            row[2], row[5] = 1., sign(r2 / r1 * third)
            row = evaluation(x0, thr)
            if taylor:
                cx, c0, c1, c2 = take(4)
                row[2], row[3], row[4], row[5], row[6], row[7], row[8], row[9], row[10], row[11] = 3., cx, c0, 1. / r1, 1. / r2, r1, r2, sign(c1), c2, r2 - r1
            else:
                cx, c0, third = take(3)
                row[2], row[3], row[4], row[5] = 2., cx, c0, sign((1. / r2) * third)
    if denoise:
        evaluation(True, thr_denoise)[2] = 7.
    rest = list(it)
    assert not rest, len(rest)
    return torch.stack(rows)


def gen():
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
    starts = {False: rnd(231, 2, 3, 32, 32), True: rnd(232, 2, 3, H, W_)}

    seen = []                                              # every vector that passes through expand_dims, in order
    plain_expand = D.expand_dims

    def recording_expand(v, dims):
        seen.append(v.reshape(-1)[0].clone())
        return plain_expand(v, dims)
    D.expand_dims = recording_expand

    def run(tag, max_val=None, dtype=torch.float32):
        """-> dict of what one reference run formed; the reference's own calls throughout."""
        skw, kw, scale = RUNS[tag]
        skw = dict(skw)
        if max_val is not None:
            skw["max_val"] = max_val
        split = tag.startswith("split")
        x_start = starts[split]
        if split:
            ld.split_input_params = dict(SPLIT)
        ns = D.NoiseScheduleVP("discrete", alphas_cumprod=ld.alphas_cumprod.clone().detach().to(dtype))
        xs, tin, rs, quant = [], [], [], []

        def apply(x, t, cc):
            xs.append(x[:x_start.shape[0]].clone())
            tin.append(t[0].clone())
            return ld.apply_model(x, t, cc)
        model_fn = D.model_wrapper(apply, ns, model_type="noise", guidance_type="classifier-free", condition=c.to(dtype),
                                   unconditional_condition=uc.to(dtype), guidance_scale=scale)
        solver = D.DPM_Solver(model_fn, ns, **skw)
        update = solver.singlestep_dpm_solver_update

        def recording_update(x, s, t, order, **k):
            rs.append((k.get("r1"), k.get("r2")))
            return update(x, s, t, order, **k)
        solver.singlestep_dpm_solver_update = recording_update
        plain_quantile = torch.quantile

        def recording_quantile(inp, q, dim=None, **k):
            out = plain_quantile(inp, q, dim=dim, **k)
            s = torch.maximum(out, solver.max_val * torch.ones_like(out))
            quant.append((out.clone(), s.clone(), bool((inp > s[:, None]).any())))
            return out
        torch.quantile = recording_quantile
        # get_orders_and_timesteps_for_singlestep_solver calls torch.cumsum without `dim` (:495), which no torch accepts, so as it
        # stands the reference's singlestep solver runs with skip_type 'logSNR' only; the sum it means is the one over dim 0
        plain_cumsum = torch.cumsum
        torch.cumsum = lambda inp, dim=0, **k: plain_cumsum(inp, dim, **k)
        del seen[:]
        try:
            out = solver.sample(x_start.to(dtype), **kw)
            method = kw.get("method", "singlestep")
            steps, order, skip = kw["steps"], kw["order"], kw.get("skip_type", "time_uniform")
            t_T, t_0 = kw.get("t_start", ns.T), kw.get("t_end", 1. / ns.total_N)
            if method == "singlestep":
                outer, orders = solver.get_orders_and_timesteps_for_singlestep_solver(steps, order, skip, t_T, t_0, "cpu")
        finally:
            torch.quantile, torch.cumsum = plain_quantile, plain_cumsum
            if split:
                del ld.split_input_params
        if method == "multistep":
            lof = kw.get("lower_order_final", True)
            orders = list(range(1, order)) + [min(order, steps + 1 - st) if (lof and steps < 15) else order for st in range(order, steps + 1)]
            outer = solver.get_time_steps(skip, t_T, t_0, steps, "cpu")
        elif method == "singlestep_fixed":
            orders = [order] * (steps // order)
            outer = solver.get_time_steps(skip, t_T, t_0, steps // order, "cpu")
        x0, thr = bool(skw.get("predict_x0", False)), bool(skw.get("thresholding", False))
        zero = torch.zeros((), dtype=dtype)
        rs = [(zero if a is None else a, zero if b is None else b) for a, b in rs]
        coef = fold(list(seen), rs, method, orders, x0, kw.get("solver_type", "dpm_solver") == "taylor", x0 and thr, thr,
                    kw.get("denoise_to_zero", False), dtype)
        assert coef.shape[0] == len(xs) == len(tin)
        res = dict(x_inter=torch.stack(xs + [out]), t_input=torch.stack(tin), timesteps=outer, orders=np.asarray(orders), coef=coef,
                   r=torch.stack([torch.stack([a, b]) for a, b in rs]) if rs else torch.zeros(0, 2, dtype=dtype))
        if quant:
            res.update(quantile=torch.stack([q[0] for q in quant]), s=torch.stack([q[1] for q in quant]),
                       max_val=np.float32(solver.max_val), clamped=np.asarray([q[2] for q in quant]))
        return res

    print(f"[G27] probe {PROBED} at max_val = 1", flush=True)
    probe = run(PROBED)["quantile"]
    max_val = {PROBED: float(f"{probe.median().item():.2g}")}
    print(f"  raw quantiles {probe.min().item():.4g} .. {probe.max().item():.4g}; max_val of {PROBED} = {max_val[PROBED]}", flush=True)

    got = {}
    for tag in RUNS:
        print(f"[G27] {tag}: {RUNS[tag]}", flush=True)
        got[tag] = run(tag, max_val.get(tag))
    thr_runs = [t for t in RUNS if "s" in got[t]]
    s_all = [(got[t]["s"], float(got[t]["max_val"])) for t in thr_runs]
    assert any(bool((s > m).any()) for s, m in s_all) and any(bool((s == m).any()) for s, m in s_all), "(a)"
    for t in thr_runs:
        assert got[t]["clamped"].any(), ("(b)", t)
        print(f"  {t}: s {got[t]['s'].min().item():.4g} .. {got[t]['s'].max().item():.4g}, max_val {float(got[t]['max_val']):.4g}, "
              f"evaluations whose clamp binds: {int(got[t]['clamped'].sum())} of {len(got[t]['clamped'])}")

    print("[G27] every run again with the whole reference in float64", flush=True)
    # the reference pins float32 in three places, lifted here in memory only (tools/make_golden_dpm.py)
    from ldm.modules.diffusionmodules.util import GroupNorm32
    ld.double()
    unet = ld.model.diffusion_model
    unet.dtype = torch.float64
    GroupNorm32.forward = torch.nn.GroupNorm.forward
    unet.time_embed.register_forward_pre_hook(lambda mod, args: (args[0].double(),))
    torch.set_default_dtype(torch.float64)
    g64 = {}
    try:
        for tag in RUNS:
            x64 = run(tag, max_val.get(tag), torch.float64)["x_inter"]
            assert x64.dtype == torch.float64
            x32 = got[tag]["x_inter"]
            d = (x64.float() - x32).abs().max().item()
            top = x32.abs().max().item()
            bound = max(1.5e-4, 4 * d)
            g64[f"{tag}_d"] = np.float32(d)
            g64[f"{tag}_final_f64"] = x64[-1].float()
            print(f"  {tag:16s} d = {d:.3e} (|x| up to {top:.2f});  bound max(1.5e-4, 4 d) = {bound:.3e} = 2^{np.log2(bound / top):.1f} |x|max",
                  flush=True)
            # a thresholded latent never leaves [-|x_T|max - 1, |x_T|max + 1] (x0 is clamped into [-1, 1]; |x_T|max = 3.71), so there
            # the floor 1.5e-4 alone is 2^-14.6 |x|max and no setting of the run can change that: held to 4 d <= 1.5e-4 instead
            floor_bound = "s" in got[tag] and 4 * d <= 1.5e-4
            assert bound <= 2.0 ** -15 * top or floor_bound, ("(c)", tag, bound, top)
    finally:
        torch.set_default_dtype(torch.float32)

    files, cur, size = [], {}, 0
    for tag in RUNS:
        nbytes = got[tag]["x_inter"].numel() * 4
        if cur and size + nbytes > FILE_BYTES:
            files.append(cur)
            cur, size = {}, 0
        for k, v in got[tag].items():
            cur[f"{tag}_{k}"] = v
        size += nbytes
    files.append(cur)
    for i, gg in enumerate(files):
        for k, v in gg.items():
            assert torch.isfinite(torch.as_tensor(v).double()).all(), k
        save(f"g27_dpm_methods_{i + 1}.npz", **gg)
    save("g27_dpm_methods_f64.npz", **g64)


if __name__ == "__main__":
    gen()
