"""First-stage encode / decode: the KL-f4 autoencoder next to the VQ-f4 one, same box, same process.

    python tools/first_stage_bench.py [--batch 16] [--image 128] [--head-only]

Timed (device events, median of 20, every shape warmed up, the two models alternating over three passes):
  encode   LatentDiffusion.encode_first_stage of a (B,3,image,image) batch -- the trunk is the same launch program for both;
           VQ ends in ldmk_conv3x3_out + ldmk_conv1x1_nchw, KL in ldmk_conv3x3_moments (and wraps the moments in a posterior)
  sample   get_first_stage_encoding of the KL posterior (ldmk_gauss_posterior + the normal draw)
  decode   decode_first_stage of a (B,3,image/4,image/4) latent, VQ with force_not_quantize=True: the same program
  head     the three boundary kernels alone on the encoder's last feature map (B, image/4, image/4, 512)
--head-only launches just the KL head a few times: the run to put under `rocprofv3 --kernel-trace --stats`."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dsml_thesis_amd import ops, synth  # noqa: E402
from rgemm_bench import timeit  # noqa: E402


def head_operands(B, hw, cin, c2z, c2e):
    torch.manual_seed(0)
    x = torch.randn(B, hw, hw, cin, device="cuda")
    gamma, beta = torch.ones(cin, device="cuda"), torch.zeros(cin, device="cuda")
    coef = ops.gn_coef(x, None, B, hw * hw, gamma, beta, 1e-6)
    w3 = ops.pack_conv3x3_narrow(torch.randn(c2z, cin, 3, 3, device="cuda") / (9 * cin) ** 0.5)
    w1 = torch.randn(c2e, c2z, device="cuda") / c2z ** 0.5
    return x, coef, w3, torch.zeros(c2z, device="cuda"), w1, torch.zeros(c2e, device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--image", type=int, default=128)
    ap.add_argument("--head-only", action="store_true")
    a = ap.parse_args()
    B, S = a.batch, a.image
    hw, cin = S // 4, 512
    x, coef, w3, b3, w1, b1 = head_operands(B, hw, cin, 6, 6)
    out = torch.empty(B, 6, hw, hw, device="cuda")
    if a.head_only:
        for _ in range(20):
            ops.conv3x3_moments(x, coef, w3, b3, w1, b1, out=out)
        torch.cuda.synchronize()
        print(f"ldmk_conv3x3_moments x20 at ({B},{hw},{hw},{cin}) -> 6 -> 6")
        return

    small = dict(synth.FR_UNET, model_channels=32, channel_mult=[1], num_res_blocks=1, attention_resolutions=[])
    kl, vq = synth.make_kl_model(unet=small), synth.make_fr_model(unet=small)
    torch.manual_seed(1)
    img = torch.tanh(torch.randn(B, 3, S, S, device="cuda"))
    z = torch.randn(B, 3, hw, hw, device="cuda")
    post = kl.encode_first_stage(img)
    print(f"B = {B}, image {S}x{S}, latent {hw}x{hw}; KL_F4 (moments 6 channels) vs VQ_F4")
    rows = []
    for rep in range(3):
        r = (timeit(lambda: kl.encode_first_stage(img)), timeit(lambda: vq.encode_first_stage(img)),
             timeit(lambda: kl.decode_first_stage(z)), timeit(lambda: vq.decode_first_stage(z, force_not_quantize=True)),
             timeit(lambda: kl.get_first_stage_encoding(post)))
        rows.append(r)
        print(f"  pass {rep}: encode KL {r[0]:9.1f} us  VQ {r[1]:9.1f} us   decode KL {r[2]:9.1f} us  VQ {r[3]:9.1f} us   "
              f"sample {r[4]:7.1f} us")
    best = [min(r[i] for r in rows) for i in range(5)]
    print(f"best of 3 medians: encode KL {best[0] / 1e3:.3f} ms, VQ {best[1] / 1e3:.3f} ms (KL - VQ {best[0] - best[1]:+.1f} us); "
          f"decode KL {best[2] / 1e3:.3f} ms, VQ {best[3] / 1e3:.3f} ms; posterior sample {best[4]:.1f} us")

    # the boundary kernels alone, on the feature map the encoder's norm_out sees
    w3v = ops.pack_conv3x3_narrow(torch.randn(3, cin, 3, 3, device="cuda") / (9 * cin) ** 0.5)
    b3v, w1v = torch.zeros(3, device="cuda"), torch.randn(3, 3, 1, 1, device="cuda")
    hz, zq = torch.empty(B, 3, hw, hw, device="cuda"), torch.empty(B, 3, hw, hw, device="cuda")
    t_head = timeit(lambda: ops.conv3x3_moments(x, coef, w3, b3, w1, b1, out=out))
    t_out = timeit(lambda: ops.conv3x3_out(x, coef, w3v, b3v, 3, out=hz))
    t_1x1 = timeit(lambda: ops.conv1x1_nchw(hz, w1v, b3v, out=zq))
    flop = 2.0 * B * hw * hw * (9 * cin * 6 + 6 * 6)
    byts = 4.0 * (x.numel() + out.numel() + w3.numel())
    print(f"ldmk_conv3x3_moments (512 -> 6 -> 6) {t_head:7.1f} us: {flop / t_head * 1e-6:.2f} TFLOP/s, {byts / t_head * 1e-3:.0f} GB/s "
          f"of input+output; grid {B * ((hw + 15) // 16) ** 2} workgroups")
    print(f"ldmk_conv3x3_out (512 -> 3) {t_out:7.1f} us + ldmk_conv1x1_nchw (3 -> 3) {t_1x1:7.1f} us = {t_out + t_1x1:7.1f} us")


if __name__ == "__main__":
    main()
