"""Timing of the noisy-latent classifier's training step on one GPU (writes profiles/classifier_timing.txt).

  python tools/classifier_bench.py [--batch 16] [--steps 100] [--rounds 3] [--pool attention] [--out profiles/classifier_timing.txt]

The shipped shape: the MEAD config's UNet turned classifier (classifier.py:95-102) -- 3 input channels at 32x32, model_channels 160,
channel_mult (1, 2, 4), two ResBlocks per level, AttentionBlocks with heads of 32 at every level, pool="attention" (an 8x8 final
grid: 65 tokens of 640 channels, 20 heads), K = 8 classes, batch 16, fp32.

Recorded:
  * the step (forward + cross-entropy + backward + AdamW): a host clock around `steps` steps that end in a device synchronise, after
    warm-up, `rounds` times (min / median / max);
  * inside one step, with device events: the head's forward launches (everything after the middle block, the cross-entropy included)
    and the head's backward closure, i.e. the head's share of the step;
  * each new kernel of csrc/classifier.hip alone at the shapes the head gives it: device events around 200 back-to-back launches,
    5 rounds after a warm-up round (min / max);
  * for context, UNetTrainer's step (p_losses + AdamW) on the full UNet with the same torso configuration.
No time is an acceptance criterion; the one expectation checked is that the head is a small share of the step."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TORSO = dict(image_size=32, in_channels=3, model_channels=160, attention_resolutions=[4, 2, 1], num_res_blocks=2,
             channel_mult=[1, 2, 4], num_head_channels=32)


def host_timed(step, steps, rounds):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    return out


def kernel_us(fn, reps=200, rounds=6):
    us = []
    for r in range(rounds):                     # (round 0 warms up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if r:
            us.append(e0.elapsed_time(e1) / reps * 1e3)
    return min(us), max(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--pool", default="attention", choices=["adaptive", "attention", "spatial", "spatial_v2"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classifier_timing.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("classifier_bench: no GPU (a timing is a GPU run or nothing)")
    from dsml_thesis_amd import schedule, synth, train_ops as T
    from dsml_thesis_amd.encoder_unet import EncoderUNetModel
    from dsml_thesis_amd.train import EncoderUNetTrainer, UNetTrainer
    from dsml_thesis_amd.unet import UNetModel
    dev = torch.device("cuda", 0)
    n, K, hw = a.batch, a.classes, TORSO["image_size"]
    gen = torch.Generator(device="cpu").manual_seed(0)
    x = torch.randn(n, 3, hw, hw, generator=gen).to(dev)
    noise = torch.randn(n, 3, hw, hw, generator=gen).to(dev)
    t = torch.randint(0, 1000, (n,), generator=gen).to(dev)
    y = torch.randint(0, K, (n,), generator=gen).to(dev)

    enc = EncoderUNetModel(**dict(TORSO, out_channels=K, pool=a.pool))
    synth.load_recipe(enc, gain=0.25)
    enc = enc.to(dev)

    class Timed(EncoderUNetTrainer):
        """Device events at the head's borders: after the middle block (forward) and around the head's closure (backward)."""
        timing = False

        def _run_torso(self, *args):
            out = super()._run_torso(*args)
            if self.timing:
                self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                self.ev[0].record()
            return out

    tr = Timed(enc)

    def step():
        logits = tr.forward(x, t)
        per, mean, dl = T.cross_entropy(logits, y)
        if tr.timing:
            tr.ev[1].record()
            fn, off = tr.tape[-1]

            def timed_head():
                tr.ev[2].record()
                fn()
                tr.ev[3].record()
            tr.tape[-1] = (timed_head, off)
        tr.backward(dl)
        tr.adamw_step(lr=1e-6)
        return mean

    for _ in range(3):
        loss = step()
    ms = host_timed(step, a.steps, a.rounds)
    head = []
    tr.timing = True
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        head.append((tr.ev[0].elapsed_time(tr.ev[1]), tr.ev[2].elapsed_time(tr.ev[3]), e0.elapsed_time(e1)))
    tr.timing = False
    hf, hb, whole = (statistics.median(v) for v in zip(*head))
    res = dict(workload=f"EncoderUNetModel pool={a.pool} fwd + cross-entropy + bwd + AdamW, fp32, batch {n}, {hw}x{hw}x3, K={K}",
               parameters=int(sum(p.numel() for p in enc.parameters())), steps=a.steps,
               step_ms_min=round(min(ms), 3), step_ms_median=round(statistics.median(ms), 3), step_ms_max=round(max(ms), 3),
               samples_per_s=round(n / (min(ms) * 1e-3), 1), head_forward_ms=round(hf, 4), head_backward_ms=round(hb, 4),
               event_timed_step_ms=round(whole, 3), head_share_of_step=round((hf + hb) / whole, 4), loss=float(loss))

    # ---- each new kernel alone, at the head's shapes
    C, g = enc._final_ch, hw // enc._final_ds
    px, heads, d = g * g, enc._final_ch // 32, 32
    act = torch.randn(n, px, C, device=dev)
    pos_t = torch.randn(px + 1, C, device=dev)
    qkv = torch.randn(n * (px + 1), 3 * C, device=dev)
    dX, dout = torch.randn(n * (px + 1), C, device=dev), torch.randn(n, C, device=dev)
    feat, dpos, dact = torch.empty(n, C, device=dev), torch.empty(px + 1, C, device=dev), torch.empty(n, px, C, device=dev)
    _, probs = T.attnpool_fwd(qkv, n, px + 1, heads, d)
    logits, hid = torch.randn(n, K, device=dev), torch.randn(n, 2048, device=dev)
    kern = {
        f"ldmk_pool_mean ({n}, {px}, {C})": lambda: T.pool_mean(act, n, px, feat=feat),
        f"ldmk_pool_mean_bwd ({n}, {px}, {C})": lambda: T.pool_mean_bwd(feat, n, px, C, dx=dact),
        f"ldmk_attnpool_tokens ({n}, {px}, {C})": lambda: T.attnpool_tokens(act.view(n * px, C), pos_t, n, px),
        f"ldmk_attnpool_tokens_bwd ({n}, {px + 1}, {C})": lambda: T.attnpool_tokens_bwd(dX, n, px, dpos_t=dpos),
        f"ldmk_attnpool_fwd ({n}, T={px + 1}, {heads} heads of {d})": lambda: T.attnpool_fwd(qkv, n, px + 1, heads, d),
        f"ldmk_attnpool_bwd ({n}, T={px + 1}, {heads} heads of {d})": lambda: T.attnpool_bwd(qkv, probs, dout, n, px + 1, heads, d),
        f"ldmk_cross_entropy ({n}, {K}), with dlogits": lambda: T.cross_entropy(logits, y),
        f"ldmk_relu ({n}, 2048)": lambda: T.relu(hid),
        f"ldmk_relu_bwd ({n}, 2048)": lambda: T.relu_bwd(hid, hid),
    }
    res["kernel_us_min_max"] = {k: [round(v, 2) for v in kernel_us(fn)] for k, fn in kern.items()}
    tr.tape, tr.G, tr.ginit, tr.last_pass = [], {}, set(), None

    # ---- context: the full UNet on the same torso configuration
    unet = UNetModel(**dict(TORSO, out_channels=3))
    synth.load_recipe(unet, gain=0.25)
    unet = unet.to(dev).eval()
    bufs = schedule.schedule_buffers(schedule.make_beta_schedule("linear", synth.SCHEDULE["timesteps"], linear_start=synth.SCHEDULE["linear_start"],
                                                                 linear_end=synth.SCHEDULE["linear_end"]), 0.0)
    sa, sb = bufs["sqrt_alphas_cumprod"].to(dev), bufs["sqrt_one_minus_alphas_cumprod"].to(dev)
    ut = UNetTrainer(unet)

    def ustep():
        ut.p_losses(x, None, t, noise, sa, sb)
        ut.adamw_step(lr=1e-6)
    for _ in range(3):
        ustep()
    ums = host_timed(ustep, a.steps, a.rounds)
    res.update(unet_parameters=int(sum(p.numel() for p in unet.parameters())), unet_step_ms_min=round(min(ums), 3),
               unet_step_ms_median=round(statistics.median(ums), 3), unet_step_ms_max=round(max(ums), 3),
               device=torch.cuda.get_device_name(0), peak_mem_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))

    lines = [f"# tools/classifier_bench.py --batch {n} --steps {a.steps} --rounds {a.rounds} --pool {a.pool} --classes {K}",
             f"# {res['device']}; host clock around {a.steps} steps ending in a synchronise, {a.rounds} rounds; kernels: device events around",
             "# 200 launches, 5 rounds after a warm-up round", "",
             res["workload"], f"  parameters                      {res['parameters']}",
             f"  step ms (min / median / max)    {res['step_ms_min']} / {res['step_ms_median']} / {res['step_ms_max']}    ({res['samples_per_s']} samples/s)",
             f"  head forward (after the middle block, cross-entropy included)   {res['head_forward_ms']} ms",
             f"  head backward (the head's closure)                              {res['head_backward_ms']} ms",
             f"  head share of the event-timed step ({res['event_timed_step_ms']} ms)                {100 * res['head_share_of_step']:.2f} %", "",
             "new kernels alone, us per launch (min / max)"]
    lines += [f"  {k:58s} {v[0]:8.2f} / {v[1]:.2f}" for k, v in res["kernel_us_min_max"].items()]
    lines += ["", f"context: UNetTrainer p_losses + AdamW on the full UNet of the same torso configuration ({res['unet_parameters']} parameters)",
              f"  step ms (min / median / max)    {res['unet_step_ms_min']} / {res['unet_step_ms_median']} / {res['unet_step_ms_max']}", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
