"""BASELINE config 5 rehearsal on one GPU: UNet training step (p_losses forward + backward + AdamW + EMA), fp32.

  python tools/train_bench.py [--batch 16] --latent 32 [--graph] [--steps 10] [--bf16] [--unet shipped|uncond|adm|heads64]
                              [--objective default|full]
--objective full: the step with the whole objective of p_losses (l1, l_simple_weight 0.8, original_elbo_weight 10, a learned
logvar with its AdamW step) on ldmk_diffusion_loss instead of the default one on ldmk_mse_grad.  Either way the result also
carries the loss stage alone, timed with device events over the pass's own output in both forms, alternating:
`loss_stage_us_default` (zeroed padded target + permute + ldmk_mse_grad) and `loss_stage_us_full` (ldmk_diffusion_loss).
--unet: the shipped spatial-transformer UNet (default), `uncond` (BASELINE configs[0]: synth.UNCOND_UNET, AttentionBlocks, no
context; 64x64x4 latent), `adm` (synth.ADM_TRAIN_UNET: scale-shift norm + class labels at the shipped widths) or `heads64` (the
shipped 64x64x4 UNet, synth.NS_UNET, with num_head_channels = 64: the flash kernels of csrc/attention_train.hip; implies
--latent 64).
Reports samples/s and the step's algorithmic TFLOP/s (3x the forward's GEMM FLOPs: forward + data-gradient + weight-
gradient products; the attention backward recomputes the scores, counted as 2.5x the forward attention FLOPs).

  python tools/train_bench.py --tune [--batch 8] [--steps 5]
The talking-face lip-reading fine-tune step (latent_tune.LatentDiffusionTune.training_step_latents: q_sample, 8 differentiable
DDIM steps at eta = 1, decode, a stand-in lip loss, backward, AdamW x3, EMA) at the tune YAML's shapes, in two forms: the DDIM
update from ldmk_ddim_diff_fwd / _bwd, and the update composed from zeros_like + ldmk_axpy chains, torch.cat and
pad_output_grad as it was before those kernels."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def axpy_ddim_class():
    """`DifferentiableDDIM` with the update composed from zeros_like + ldmk_axpy chains, torch.cat and pad_output_grad, as it
    was before csrc/ddim_diff.hip: the other side of the --tune timing, and the reference of
    tests/test_tune_gpu.py::test_eta0_walk_equals_the_axpy_composition (the one copy of that arithmetic)."""
    from dsml_thesis_amd import train_ops as T
    from dsml_thesis_amd.train import UNetTrainer
    from dsml_thesis_amd.train_decoder import DifferentiableDDIM, lincomb

    class AxpyDDIM(DifferentiableDDIM):
        def forward(self, x, c, table, timesteps, scale=1.0, uc=None, noise=None, c_concat=None):
            self.passes, tr, x = [], self.tr, x.float()
            n, self._C = x.shape[0], x.shape[1]
            cfg = uc is not None and scale != 1.0
            for k, i in enumerate(reversed(range(len(timesteps)))):
                a_t, a_prev, sigma, s1m = (float(v) for v in table[i])
                ts = torch.full((n,), int(timesteps[i]), device=x.device, dtype=torch.long)
                xin = x if c_concat is None else torch.cat([x, c_concat.float()], 1)
                if cfg:
                    eps2 = tr.forward(torch.cat([xin, xin]), torch.cat([ts, ts]), torch.cat([uc, c]))
                    e_t = lincomb([(1.0 - scale, eps2[:n]), (scale, eps2[n:])])
                else:
                    e_t = tr.forward(xin, ts, c)
                cx = (a_prev / a_t) ** 0.5
                ce = (1.0 - a_prev - sigma * sigma) ** 0.5 - cx * s1m
                self.passes.append((tr.last_pass, cx, ce, cfg, scale, n))
                terms = [(cx, x), (ce, e_t)]
                if sigma != 0.0:
                    terms.append((sigma, torch.randn_like(x) if noise is None else noise[k]))
                x = lincomb(terms)
            self.z, self._ctx_shape = x, tuple(c.shape)
            return self.dec.forward(lincomb([(1.0 / float(self.model.scale_factor), x)]))

        def backward(self, dimg, dz=None):
            tr, C = self.tr, self._C
            dx = lincomb([(1.0 / float(self.model.scale_factor), self.dec.backward(dimg))])
            if dz is not None:
                T.axpy_(dx, dz.float().contiguous(), 1.0)
            tr.P.grad.zero_()
            old, d = (tr.acc_params, tr.want_dx), None
            tr.acc_params, tr.want_dx = True, True
            try:
                for ps, cx, ce, cfg, scale, n in reversed(self.passes):
                    if cfg:
                        deps = torch.cat([lincomb([(ce * (1.0 - scale), dx)]), lincomb([(ce * scale, dx)])])
                        dxin = tr.backward(UNetTrainer.pad_output_grad(deps), ps)
                        dx = lincomb([(cx, dx), (1.0, dxin[:n, :C].contiguous()), (1.0, dxin[n:, :C].contiguous())])
                    else:
                        dxin = tr.backward(UNetTrainer.pad_output_grad(lincomb([(ce, dx)])), ps)
                        dx = lincomb([(cx, dx), (1.0, dxin[:, :C].contiguous())])
                    rows = ps["dctx"][-(ps["dctx"].shape[0] // (2 if cfg else 1)):]
                    d = rows.clone() if d is None else d.add_(rows)
            finally:
                tr.acc_params, tr.want_dx = old
            self.d_context, self.passes = d.view(self._ctx_shape), []
            return dx
    return AxpyDDIM


def tune_bench(a):
    import torch.nn.functional as F
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.train_decoder import DifferentiableDDIM
    from dsml_thesis_amd.util import instantiate_from_config
    AxpyDDIM = axpy_ddim_class()

    dev = torch.device("cuda", 0)
    cfg = synth.tf_config(seq_len=9)
    cfg.update(lr_loss_w=1.0, start_lr_loss=0)
    model = instantiate_from_config({"target": "ldm.models.diffusion.ddpm2condtune.LatentDiffusion", "params": cfg})
    synth.load_recipe(model.model.diffusion_model, gain=0.25)
    for m in (model.first_stage_model, model.cond_stage_model_1, model.cond_stage_model_2):
        synth.load_recipe(m)
    model = model.to(dev).train()
    g = torch.Generator(device="cpu").manual_seed(0)
    w = (0.2 * torch.randn(8, 3, 3, 3, generator=g)).to(dev)

    def lip_loss(x, x0, l):                      # stand-in for the lip-reading network: conv feature of a mouth-region crop
        fa, fb = (F.avg_pool2d(F.conv2d(im[:, :, 72:120, 32:96], w), 4).flatten(1) for im in (x0, x))
        return 1 - F.cosine_similarity(fa, fb, dim=1).mean()
    model.lip_loss_func = lip_loss
    n = a.batch or 8                             # the tune YAML's batch size
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)
    args = dict(x=rn(n, 3, 32, 32), c1={"class_label": torch.randint(0, 8, (n,), generator=g).to(dev)}, c2=rn(n, 9, 768),
                c3=rn(n, 3, 32, 32), c4=rn(n, 3, 32, 32), l=torch.zeros(n, 20, 2, device=dev),
                t=torch.randint(0, 1000, (n,), generator=g).to(dev), noise=rn(n, 3, 32, 32),
                ddim_noise=[rn(n, 3, 32, 32) for _ in range(model.num_tune_steps)])
    res = dict(workload=f"talking-face lip-reading fine-tune step fp32, batch {n}, latent 32, 8 DDIM steps eta 1", steps=a.steps)
    for form, cls in (("kernels", DifferentiableDDIM), ("axpy", AxpyDDIM), ("kernels_again", DifferentiableDDIM)):
        model._ddd = cls(model)
        for _ in range(2):
            loss, _ = model.training_step_latents(lr=1e-6, **args)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            loss, _ = model.training_step_latents(lr=1e-6, **args)
        torch.cuda.synchronize()
        res[f"ms_per_step_{form}"] = round((time.perf_counter() - t0) / a.steps * 1e3, 2)
        res[f"loss_{form}"] = float(loss)
    res["peak_mem_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=None, help="default 16 (8 with --tune)")
    ap.add_argument("--tune", action="store_true", help="time the talking-face lip-reading fine-tune step instead")
    ap.add_argument("--latent", type=int, default=32, choices=[32, 64])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--bf16", action="store_true", help="bf16 GEMM operands (UNetTrainer compute='bf16')")
    ap.add_argument("--unet", default="shipped", choices=["shipped", "uncond", "adm", "heads64"])
    ap.add_argument("--objective", default="default", choices=["default", "full"])
    a = ap.parse_args()
    if a.tune:
        return tune_bench(a)
    a.batch = a.batch or 16
    if a.unet == "heads64":
        a.latent = 64
    from dsml_thesis_amd.train import UNetTrainer
    dev = torch.device("cuda", 0)
    if a.unet == "shipped":
        from bench import build_model
        model, ucfg = build_model(a.latent, dev)
        unet = model.model.diffusion_model
        sa, sb = model.sqrt_alphas_cumprod, model.sqrt_one_minus_alphas_cumprod
    else:
        from dsml_thesis_amd import schedule, synth
        from dsml_thesis_amd.unet import UNetModel
        ch = 4 if a.latent == 64 else 3
        if a.unet == "heads64":
            ucfg = dict(synth.NS_UNET, num_head_channels=64)
        else:
            ucfg = dict(synth.UNCOND_UNET if a.unet == "uncond" else synth.ADM_TRAIN_UNET, image_size=a.latent, in_channels=ch,
                        out_channels=ch)
        unet = UNetModel(**ucfg)
        synth.load_recipe(unet, gain=0.25)
        unet = unet.to(dev).eval()
        bufs = schedule.schedule_buffers(schedule.make_beta_schedule("linear", synth.SCHEDULE["timesteps"],
                                                                     linear_start=synth.SCHEDULE["linear_start"],
                                                                     linear_end=synth.SCHEDULE["linear_end"]), 0.0)
        sa, sb = bufs["sqrt_alphas_cumprod"].to(dev), bufs["sqrt_one_minus_alphas_cumprod"].to(dev)
    from dsml_thesis_amd import schedule as S_, synth as Y_, train_ops as T
    lvlb = S_.schedule_buffers(S_.make_beta_schedule("linear", Y_.SCHEDULE["timesteps"], linear_start=Y_.SCHEDULE["linear_start"],
                                                     linear_end=Y_.SCHEDULE["linear_end"]), 0.0, "eps")["lvlb_weights"].to(dev)
    logvar = torch.full((lvlb.numel(),), -0.7, device=dev)
    lv_m, lv_v = torch.zeros_like(logvar), torch.zeros_like(logvar)
    full = dict(parameterization="eps", loss_type="l1", l_simple_weight=0.8, original_elbo_weight=10., logvar=logvar,
                lvlb_weights=lvlb, learn_logvar=True)
    tr = UNetTrainer(unet, compute="bf16" if a.bf16 else "f32")
    n, c, hw = a.batch, ucfg["in_channels"], a.latent
    g = torch.Generator(device="cpu").manual_seed(0)
    x0 = torch.randn(n, c, hw, hw, generator=g).to(dev)
    noise = torch.randn(n, ucfg["out_channels"], hw, hw, generator=g).to(dev)
    ctx = torch.randn(n, 1, ucfg["context_dim"], generator=g).to(dev) if ucfg.get("context_dim") else None
    y = torch.randint(0, ucfg["num_classes"], (n,), generator=g).to(dev) if ucfg.get("num_classes") else None
    t = torch.randint(0, 1000, (n,), generator=g).to(dev)
    shadow = tr.P.flat.clone()
    loss_buf = torch.zeros(1, device=dev)

    def step():
        loss = tr.p_losses(x0, ctx, t, noise, sa, sb, y=y, objective=full if a.objective == "full" else None)
        tr.adamw_step(lr=1e-6)
        if a.objective == "full":
            T.adamw_(logvar, tr.objective_out["dlogvar"], lv_m, lv_v, 1e-6, (0.9, 0.999), 1e-8, 1e-2, tr.P.step)
        tr.ema_update(shadow, 0.9999)
        loss_buf.copy_(loss)

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    run = step
    if a.graph:
        tr.P.step = 2          # the bias corrections are host scalars: freeze them for the captured replay
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            step()
        run = gr.replay
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    res = dict(workload=f"UNet p_losses fwd+bwd+AdamW+EMA {'bf16' if a.bf16 else 'fp32'}, batch {n}, latent {hw}", unet=a.unet,
               graph=a.graph, steps=a.steps, ms_per_step=round(dt * 1e3, 2), samples_per_s=round(n / dt, 2))
    if a.unet == "shipped":                 # (the FLOP counts below are the shipped UNet's)
        fwd_gemm = (42.17 if a.latent == 32 else 168.62) * 1e9 * n
        fwd_attn = (3.84 if a.latent == 32 else 61.43) * 1e9 * n
        res["step_tflops"] = round((3 * fwd_gemm + 3.5 * fwd_attn) / dt / 1e12, 1)
    # the loss stage alone, over the output of one more forward pass, both forms in turn
    tr.forward(x0, t, ctx, y=y)
    co = noise.shape[1]

    def stage_default():
        tgt = torch.zeros_like(tr.eps_pad)
        tgt[..., :co] = noise.permute(0, 2, 3, 1)
        T.mse_grad(tr.eps_pad, tgt, denom=noise.numel())

    def stage_full():
        T.diffusion_loss(tr.eps_pad, noise, t, logvar, lvlb, "l1", 0.8, 10.)
    us = dict(default=[], full=[])
    for rnd_ in range(6):                   # (round 0 warms both up)
        for name, fn in (("default", stage_default), ("full", stage_full)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if rnd_:
                us[name].append(e0.elapsed_time(e1) / 200 * 1e3)
    res.update(objective=a.objective, loss_stage_us_default=round(min(us["default"]), 1), loss_stage_us_full=round(min(us["full"]), 1),
               loss_stage_us_default_max=round(max(us["default"]), 1), loss_stage_us_full_max=round(max(us["full"]), 1))
    tr.tape, tr.G, tr.ginit, tr.last_pass = [], {}, set(), None
    res.update(loss=float(loss_buf.item()), peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
