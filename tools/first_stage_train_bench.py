"""One VQGAN autoencoder training step on the HIP trainer next to the same step on PyTorch-ROCm autograd, same box, same process.

    python tools/first_stage_train_bench.py [--batch 16] [--iters 10]

Workload: the shipped VQ-f4 (synth.VQ_F4: ch 128, [1, 2, 4], 128x128, 16384 codes), recipe weights, l2 pixel loss + codebook
loss.  Timed with device events, median of `iters`, every shape warmed up, the two sides alternating over three passes:
  forward / backward / adam   FirstStageTrainer.forward, .backward (every parameter gradient), .adam_step
  kernels                     ldmk_vq_loss_bwd, ldmk_vq_codebook_grad, ldmk_conv1x1_nchw_bwd, ldmk_l1_grad alone at the step's shapes
  torch                       the oracle's encoder / quantiser / decoder restatement as torch ops on the GPU: forward, backward
                              (autograd), torch.optim.Adam(betas=(0.5, 0.9)) over the same parameters"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dsml_thesis_amd import ops, synth, train_ops as T  # noqa: E402
from dsml_thesis_amd.train_first_stage import FirstStageTrainer  # noqa: E402
from oracle import ldm_oracle as O  # noqa: E402
from rgemm_bench import timeit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    cfg, B = synth.VQ_F4, a.batch
    dd = cfg["ddconfig"]
    S = dd["resolution"]
    vq = synth.make_vq_first_stage(cfg)
    tr = FirstStageTrainer(vq)
    torch.manual_seed(1)
    x = torch.tanh(torch.randn(B, 3, S, S, device="cuda"))
    params = {k: torch.nn.Parameter(v.detach().clone()) for k, v in vq.state_dict().items()}
    opt = torch.optim.Adam(list(params.values()), lr=1e-6, betas=(0.5, 0.9))
    st = {}

    def hip_fwd():
        st["xrec"] = tr.forward(x)

    def hip_bwd():                      # needs the tape of a forward: timed as (forward + backward) - forward
        hip_fwd()
        _, d = T.mse_grad(st["xrec"], x)
        tr.backward(d, codebook_weight=1.0)

    def torch_fwd():
        with torch.enable_grad():
            z = F.conv2d(O.encoder_forward(params, dd, x), params["quant_conv.weight"], params["quant_conv.bias"])
            cb = params["quantize.embedding.weight"]
            _, idx = ops.vq_nearest(z.detach().contiguous(), cb.detach())          # the search is not what is compared
            e = cb[idx.reshape(-1).long()].view(B, z.shape[2], z.shape[3], -1).permute(0, 3, 1, 2)
            q = torch.mean((e.detach() - z) ** 2) + 0.25 * torch.mean((e - z.detach()) ** 2)
            xrec = O.decoder_forward(params, dd, F.conv2d(z + (e - z).detach(), params["post_quant_conv.weight"],
                                                          params["post_quant_conv.bias"]))
            st["loss"] = torch.mean((xrec - x) ** 2) + q

    def torch_bwd():
        torch_fwd()
        opt.zero_grad(set_to_none=True)
        st["loss"].backward()

    hip_bwd()
    torch_bwd()
    rows = []
    for _ in range(3):
        rows.append((timeit(hip_fwd, a.iters), timeit(hip_bwd, a.iters), timeit(lambda: tr.adam_step(1e-6), a.iters),
                     timeit(torch_fwd, a.iters), timeit(torch_bwd, a.iters), timeit(opt.step, a.iters)))
    hf, hfb, ha, tf, tfb, ta = (sorted(c)[1] for c in zip(*rows))
    n_par = sum(p.numel() for p in params.values())
    print(f"VQ-f4 training step, B = {B}, {S}x{S}, {n_par / 1e6:.1f} M parameters (median of 3 passes x {a.iters} runs)")
    print(f"  HIP trainer : forward {hf / 1e3:8.2f} ms  backward {(hfb - hf) / 1e3:8.2f} ms  adam {ha / 1e3:7.3f} ms  step {(hfb + ha) / 1e3:8.2f} ms")
    print(f"  torch       : forward {tf / 1e3:8.2f} ms  backward {(tfb - tf) / 1e3:8.2f} ms  adam {ta / 1e3:7.3f} ms  step {(tfb + ta) / 1e3:8.2f} ms")
    print(f"  step ratio torch / HIP = {(tfb + ta) / (hfb + ha):.2f}")
    z, cb, idx = tr.z, tr.P.p["quantize.embedding.weight"], tr.idx
    dzq = torch.randn_like(z)
    hz = torch.randn_like(z)
    w11 = tr.P.p["quant_conv.weight"]
    t1 = timeit(lambda: T.vq_loss_bwd(z, cb, idx, dzq=dzq))
    t2 = timeit(lambda: T.vq_codebook_grad(z, cb, idx))
    t3 = timeit(lambda: T.conv1x1_nchw_bwd(hz, dzq, w11))
    t4 = timeit(lambda: T.l1_grad(st["xrec"], x))
    step_us = hfb + ha
    print(f"  kernels at {tuple(z.shape)} latents, {cb.shape[0]} codes, {idx.numel()} rows (wrappers included):")
    for name, t in (("ldmk_vq_loss_bwd", t1), ("ldmk_vq_codebook_grad", t2), ("ldmk_conv1x1_nchw_bwd", t3), ("ldmk_l1_grad", t4)):
        print(f"    {name:24s} {t:8.1f} us  {100 * t / step_us:6.3f} % of the step")


if __name__ == "__main__":
    main()
