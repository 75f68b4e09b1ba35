"""One first-stage autoencoder training step on the HIP trainer next to the same step on PyTorch-ROCm autograd, same box, same
process: the VQGAN's, or with --kl the KL autoencoder's.

    python tools/first_stage_train_bench.py [--kl] [--batch 16] [--iters 10] [--out profiles/kl_train_timing.txt]

Workload: the shipped VQ-f4 (synth.VQ_F4: ch 128, [1, 2, 4], 128x128, 16384 codes), recipe weights, l2 pixel loss + codebook
loss.  Timed with device events, median of `iters`, every shape warmed up, the two sides alternating over three passes:
  forward / backward / adam   FirstStageTrainer.forward, .backward (every parameter gradient), .adam_step
  kernels                     ldmk_vq_loss_bwd, ldmk_vq_codebook_grad, ldmk_conv1x1_nchw_bwd, ldmk_l1_grad alone at the step's shapes
  torch                       the oracle's encoder / quantiser / decoder restatement as torch ops on the GPU: forward, backward
                              (autograd), torch.optim.Adam(betas=(0.5, 0.9)) over the same parameters
--kl: the KL-f4 autoencoder (synth.KL_F4: the same trunk, a 6-channel moment head), sampled posterior from one fixed noise, the
L1 term of the NLL at logvar 0 plus kl_weight 1e-6 times the mean KL, timed the same way; the kernels timed alone are
ldmk_gauss_kl_fwd, ldmk_gauss_kl_bwd, ldmk_l1_sum_grad and the 6 <-> 6 ldmk_conv1x1_nchw_bwd.  The report is printed and, with
--kl, also written to --out."""
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


def _report(name, B, S, n_par, iters, rows):
    hf, hfb, ha, tf, tfb, ta = (sorted(c)[1] for c in zip(*rows))
    return [f"{name} training step, B = {B}, {S}x{S}, {n_par / 1e6:.1f} M parameters (median of 3 passes x {iters} runs)",
            f"  HIP trainer : forward {hf / 1e3:8.2f} ms  backward {(hfb - hf) / 1e3:8.2f} ms  adam {ha / 1e3:7.3f} ms  step {(hfb + ha) / 1e3:8.2f} ms",
            f"  torch       : forward {tf / 1e3:8.2f} ms  backward {(tfb - tf) / 1e3:8.2f} ms  adam {ta / 1e3:7.3f} ms  step {(tfb + ta) / 1e3:8.2f} ms",
            f"  step ratio torch / HIP = {(tfb + ta) / (hfb + ha):.2f}"], hfb + ha


def main_kl(a):
    cfg, B, KLW = synth.KL_F4, a.batch, 1e-6
    dd, e = cfg["ddconfig"], cfg["embed_dim"]
    S = dd["resolution"]
    kl = synth.make_kl_first_stage(cfg)
    tr = FirstStageTrainer(kl)
    torch.manual_seed(1)
    x = torch.tanh(torch.randn(B, 3, S, S, device="cuda"))
    noise = torch.randn(B, e, S // 4, S // 4, device="cuda")
    params = {k: torch.nn.Parameter(v.detach().clone()) for k, v in kl.state_dict().items()}
    opt = torch.optim.Adam(list(params.values()), lr=1e-6, betas=(0.5, 0.9))
    st = {}

    def hip_fwd():
        st["xrec"] = tr.forward(x, noise=noise)

    def hip_bwd():                      # needs the tape of a forward: timed as (forward + backward) - forward
        hip_fwd()
        _, d = T.l1_sum_grad(st["xrec"], x, 1.0 / B)
        tr.backward(d, kl_weight=KLW)

    def torch_fwd():
        with torch.enable_grad():
            mom = F.conv2d(O.encoder_forward(params, dd, x), params["quant_conv.weight"], params["quant_conv.bias"])
            mean, lv = torch.chunk(mom, 2, dim=1)
            lv = torch.clamp(lv, -30.0, 20.0)
            z = mean + torch.exp(0.5 * lv) * noise
            klb = 0.5 * torch.sum(mean ** 2 + torch.exp(lv) - 1.0 - lv, dim=[1, 2, 3])
            xrec = O.decoder_forward(params, dd, F.conv2d(z, params["post_quant_conv.weight"], params["post_quant_conv.bias"]))
            st["loss"] = (xrec - x).abs().sum() / B + KLW * klb.sum() / B

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
    lines, step_us = _report("KL-f4", B, S, sum(p.numel() for p in params.values()), a.iters, rows)
    mom, z = tr.moments, tr.z
    dz, dmom, hz = torch.randn_like(z), torch.randn_like(mom), torch.randn_like(mom)
    t1 = timeit(lambda: T.gauss_kl_fwd(mom, noise))
    t2 = timeit(lambda: T.gauss_kl_bwd(mom, noise, dz, KLW / B))
    t3 = timeit(lambda: T.l1_sum_grad(st["xrec"], x, 1.0 / B))
    t4 = timeit(lambda: T.conv1x1_nchw_bwd(hz, dmom, tr.P.p["quant_conv.weight"]))
    lines.append(f"  kernels at {tuple(mom.shape)} moments, {tuple(x.shape)} images (wrappers included):")
    for name, t in (("ldmk_gauss_kl_fwd", t1), ("ldmk_gauss_kl_bwd", t2), ("ldmk_l1_sum_grad", t3), ("ldmk_conv1x1_nchw_bwd 6<->6", t4)):
        lines.append(f"    {name:28s} {t:8.1f} us  {100 * t / step_us:6.3f} % of the step")
    print("\n".join(lines))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--kl", action="store_true", help="the KL-f4 autoencoder's step instead of the VQGAN's")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "kl_train_timing.txt"))
    a = ap.parse_args()
    if a.kl:
        return main_kl(a)
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
    lines, step_us = _report("VQ-f4", B, S, sum(p.numel() for p in params.values()), a.iters, rows)
    print("\n".join(lines))
    z, cb, idx = tr.z, tr.P.p["quantize.embedding.weight"], tr.idx
    dzq = torch.randn_like(z)
    hz = torch.randn_like(z)
    w11 = tr.P.p["quant_conv.weight"]
    t1 = timeit(lambda: T.vq_loss_bwd(z, cb, idx, dzq=dzq))
    t2 = timeit(lambda: T.vq_codebook_grad(z, cb, idx))
    t3 = timeit(lambda: T.conv1x1_nchw_bwd(hz, dzq, w11))
    t4 = timeit(lambda: T.l1_grad(st["xrec"], x))
    print(f"  kernels at {tuple(z.shape)} latents, {cb.shape[0]} codes, {idx.numel()} rows (wrappers included):")
    for name, t in (("ldmk_vq_loss_bwd", t1), ("ldmk_vq_codebook_grad", t2), ("ldmk_conv1x1_nchw_bwd", t3), ("ldmk_l1_grad", t4)):
        print(f"    {name:24s} {t:8.1f} us  {100 * t / step_us:6.3f} % of the step")


if __name__ == "__main__":
    main()
