"""BASELINE config 5 rehearsal on one GPU: UNet training step (p_losses forward + backward + AdamW + EMA), fp32.

  python tools/train_bench.py --batch 16 --latent 32 [--graph] [--steps 10] [--bf16] [--unet shipped|uncond|adm|heads64]
--unet: the shipped spatial-transformer UNet (default), `uncond` (BASELINE configs[0]: synth.UNCOND_UNET, AttentionBlocks, no
context; 64x64x4 latent), `adm` (synth.ADM_TRAIN_UNET: scale-shift norm + class labels at the shipped widths) or `heads64` (the
shipped 64x64x4 UNet, synth.NS_UNET, with num_head_channels = 64: the flash kernels of csrc/attention_train.hip; implies
--latent 64).
Reports samples/s and the step's algorithmic TFLOP/s (3x the forward's GEMM FLOPs: forward + data-gradient + weight-
gradient products; the attention backward recomputes the scores, counted as 2.5x the forward attention FLOPs)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--latent", type=int, default=32, choices=[32, 64])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--bf16", action="store_true", help="bf16 GEMM operands (UNetTrainer compute='bf16')")
    ap.add_argument("--unet", default="shipped", choices=["shipped", "uncond", "adm", "heads64"])
    a = ap.parse_args()
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
        loss = tr.p_losses(x0, ctx, t, noise, sa, sb, y=y)
        tr.adamw_step(lr=1e-6)
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
    res.update(loss=float(loss_buf.item()), peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
