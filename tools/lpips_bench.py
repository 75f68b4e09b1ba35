"""LPIPS (VGG16) value + image gradient on HIP next to the same on PyTorch-ROCm autograd, same box, same process, and what it
adds to a KL first-stage training iteration.

    python tools/lpips_bench.py [--batch 16] [--iters 10] [--sizes 128 256] [--out profiles/lpips_timing.txt]

Synthetic weights (synth.lpips_state_dict), images uniform in [-1, 1], the reconstruction the image plus 0.2 noise, clamped.
Timed with device events, median of `iters` runs, every shape warmed up, the two sides alternating over three passes (the median
pass is reported):
  HIP        LPIPS.value_and_grad(input, target): the value and the gradient with respect to the target; and the value alone
  torch      a plain torch module with the same weights (F.conv2d / F.max_pool2d, the reference's arithmetic), forward under
             autograd and backward to the target; and the value alone under no_grad
  accuracy   both against that torch module in float64 on the GPU, same inputs.  With thousands of tap pixels a few have an almost
             all-zero feature vector, where 1 / |f| makes the gradient ill-conditioned: there fp32 of either side is percent-level
             off float64 in the maximum norm and 1e-3 in rms, HIP and torch alike
  families   the HIP call again with a device-event pair around every launch wrapper, summed per kernel family: the boundary
             convolution (ldmk_lpips_conv_in and its backward), the twelve forward GEMMs, their twelve data-gradient GEMMs, the
             standalone ReLU passes (ldmk_relu, ldmk_relu_bwd), ReLU + max-pool and its backward, the LPIPS layer kernels.  The
             families do not add up to the whole: the remainder is the host time between launches that the device waits for.
  train      AutoencoderKL.train_batch on KL-f4 (synth.KL_F4, 128 x 128, both optimizers' steps, PatchGAN of 3 layers) with the
             HIP LPIPS as the perceptual network and with losses.StandInPerceptual, alternating
The report is printed and written to --out."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dsml_thesis_amd import ops, synth, train_ops as T  # noqa: E402
from dsml_thesis_amd.lpips import LPIPS  # noqa: E402
from rgemm_bench import timeit  # noqa: E402

KL_TARGET = "ldm.modules.losses.contperceptual.LPIPSWithDiscriminator"
FAMILIES = (("boundary conv (conv_in, conv_in_bwd)", T, ("lpips_conv_in", "lpips_conv_in_bwd")),
            ("forward GEMMs (ops.conv3x3)", ops, ("conv3x3",)),
            ("dgrad GEMMs (conv3x3_dgrad)", T, ("conv3x3_dgrad",)),
            ("standalone ReLU passes (relu, relu_bwd)", T, ("relu", "relu_bwd")),
            ("ReLU + max-pool, and backward", T, ("relu_maxpool2", "relu_maxpool2_bwd")),
            ("LPIPS layer kernels (fwd, bwd)", T, ("lpips_layer", "lpips_layer_bwd")))


def vgg_flops(h, w):
    """multiply-adds x 2 of the thirteen convolutions for one image, forward"""
    total = 0
    for k, convs in synth.LPIPS_VGG:
        hh, ww = h >> (k - 1), w >> (k - 1)
        total += sum(2 * 9 * cin * cout * hh * ww for _, cin, cout in convs)
    return total


class TorchLPIPS(torch.nn.Module):
    def __init__(self, sd):
        super().__init__()
        self.sd = {k: v.cuda() for k, v in sd.items()}
        self.lin = [v.cuda() for k, v in sd.items() if k.startswith("lin")]

    def features(self, x):
        h = (x - self.sd["scaling_layer.shift"]) / self.sd["scaling_layer.scale"]
        taps = []
        for k, convs in synth.LPIPS_VGG:
            if k > 1:
                h = F.max_pool2d(h, 2, 2)
            for i, _, _ in convs:
                h = F.relu(F.conv2d(h, self.sd[f"net.slice{k}.{i}.weight"], self.sd[f"net.slice{k}.{i}.bias"], padding=1))
            taps.append(h)
        return taps

    def forward(self, a, b):
        val = 0
        for f0, f1, w in zip(self.features(a), self.features(b), self.lin):
            u0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
            u1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
            val = val + F.conv2d((u0 - u1) ** 2, w).mean([2, 3], keepdim=True)
        return val


def family_times(net, x, y, iters):
    """per-family device time (us) of one value_and_grad: every wrapper call between its own pair of events"""
    sums = {name: [] for name, _, _ in FAMILIES}
    saved = []
    for name, mod, fns in FAMILIES:
        for fn in fns:
            orig = getattr(mod, fn)
            saved.append((mod, fn, orig))

            def timed(*a, _orig=orig, _name=name, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = _orig(*a, **kw)
                e1.record()
                pairs[_name].append((e0, e1))
                return r
            setattr(mod, fn, timed)
    try:
        for it in range(iters + 2):
            pairs = {name: [] for name, _, _ in FAMILIES}
            net.value_and_grad(x, y)
            torch.cuda.synchronize()
            if it >= 2:
                for name in sums:
                    sums[name].append(sum(e0.elapsed_time(e1) for e0, e1 in pairs[name]) * 1e3)
        counts = {name: len(p) for name, p in pairs.items()}
    finally:
        for mod, fn, orig in saved:
            setattr(mod, fn, orig)
    return {name: float(np.median(v)) for name, v in sums.items()}, counts


def bench_size(net, tnet, B, S, iters):
    rs = np.random.RandomState(S)
    x = torch.from_numpy(rs.uniform(-1, 1, (B, 3, S, S)).astype(np.float32)).cuda()
    y = (x + 0.2 * torch.from_numpy(rs.standard_normal((B, 3, S, S)).astype(np.float32)).cuda()).clamp(-1, 1)

    def hip_vg():
        net.value_and_grad(x, y)

    def hip_v():
        with torch.no_grad():
            net(x, y)

    def torch_vg():
        leaf = y.clone().requires_grad_(True)
        torch.autograd.grad(tnet(x, leaf).sum(), leaf)

    def torch_v():
        with torch.no_grad():
            tnet(x, y)

    # both fp32 sides against the same module in float64 on the GPU (torch's native double convolution), on these inputs
    t64 = TorchLPIPS({k: v.double() for k, v in tnet.sd.items()})
    l64 = y.double().requires_grad_(True)
    v_r = t64(x.double(), l64)
    g_r, = torch.autograd.grad(v_r.sum(), l64)
    v_h, g_h = net.value_and_grad(x, y)
    leaf = y.clone().requires_grad_(True)
    v_t = tnet(x, leaf)
    g_t, = torch.autograd.grad(v_t.sum(), leaf)

    def dev(a, b):
        return ((a.double() - b).abs().max() / b.abs().max()).item()

    def dev_rms(a, b):
        return ((a.double() - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()
    acc = (f"  against float64 on the GPU (max abs / max abs; rms / rms): HIP value {dev(v_h, v_r):.2e}, gradient {dev(g_h, g_r):.2e}; "
           f"{dev_rms(g_h, g_r):.2e} -- torch fp32 value {dev(v_t, v_r):.2e}, gradient {dev(g_t, g_r):.2e}; {dev_rms(g_t, g_r):.2e}")
    del t64, l64, v_r, g_r
    rows = [(timeit(hip_vg, iters), timeit(hip_v, iters), timeit(torch_vg, iters), timeit(torch_v, iters)) for _ in range(3)]
    hvg, hv, tvg, tv = (sorted(c)[1] for c in zip(*rows))
    fl = vgg_flops(S, S) * B
    lines = [f"LPIPS (VGG16) B = {B}, {S}x{S}: {fl * 2 / 1e9:.1f} GFLOP forward (two branches), {fl * 3 / 1e9:.1f} GFLOP value + target gradient "
             f"(median of 3 passes x {iters} runs)",
             f"  HIP   : value + gradient {hvg / 1e3:8.2f} ms ({fl * 3 / hvg / 1e6:6.1f} TFLOP/s end to end)   value alone {hv / 1e3:8.2f} ms",
             f"  torch : value + gradient {tvg / 1e3:8.2f} ms ({fl * 3 / tvg / 1e6:6.1f} TFLOP/s end to end)   value alone {tv / 1e3:8.2f} ms",
             f"  ratio torch / HIP = {tvg / hvg:.2f} (value + gradient), {tv / hv:.2f} (value alone)",
             acc]
    fam, counts = family_times(net, x, y, iters)
    total = sum(fam.values())
    lines.append(f"  kernel families of one HIP value + gradient (events around every wrapper; sum {total / 1e3:.2f} ms of {hvg / 1e3:.2f} ms):")
    for name, t in fam.items():
        lines.append(f"    {name:42s} {counts[name]:3d} calls {t / 1e3:8.3f} ms  {100 * t / total:5.1f} % of the sum")
    return lines


def bench_train(sd, B, iters):
    from dsml_thesis_amd.autoencoder import AutoencoderKL
    from dsml_thesis_amd.losses import StandInPerceptual
    cfg = synth.KL_F4
    S = cfg["ddconfig"]["resolution"]
    models = {}
    for name in ("stand-in", "HIP LPIPS"):
        if name == "stand-in":
            perceptual = StandInPerceptual(5)
        else:
            perceptual = LPIPS()
            perceptual.load_state_dict(sd)
        torch.manual_seed(11)
        m = AutoencoderKL(ddconfig=dict(cfg["ddconfig"]), embed_dim=cfg["embed_dim"],
                          lossconfig=dict(target=KL_TARGET, params=dict(disc_start=0, kl_weight=1e-6, disc_weight=0.5,
                                                                        perceptual_weight=1.0, perceptual_loss=perceptual)))
        own = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("loss.") and v.dtype.is_floating_point and v.dim() > 0}
        m.load_state_dict(synth.synth_state_dict(own), strict=False)
        m = m.cuda()
        m.learning_rate = 1e-6
        models[name] = m
    rs = np.random.RandomState(3)
    batch = dict(image=torch.from_numpy(np.tanh(rs.standard_normal((B, S, S, 3))).astype(np.float32)).cuda())
    rows = [tuple(timeit(lambda m=m: m.train_batch(batch), iters) for m in models.values()) for _ in range(3)]
    t_s, t_l = (sorted(c)[1] for c in zip(*rows))
    finite = all(torch.isfinite(torch.as_tensor(v)).all() for v in models["HIP LPIPS"].logged.values() if torch.is_tensor(v))
    return [f"AutoencoderKL.train_batch, KL-f4, B = {B}, {S}x{S}, both optimizers' steps (median of 3 passes x {iters} runs)",
            f"  with losses.StandInPerceptual : {t_s / 1e3:8.2f} ms",
            f"  with lpips.LPIPS on HIP       : {t_l / 1e3:8.2f} ms   (+{(t_l - t_s) / 1e3:.2f} ms, x{t_l / t_s:.2f}; logs finite: {finite})",
            "  (profiles/kl_train_timing.txt: 123.24 ms for the trainer's forward + backward + Adam alone, no loss class)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lpips_timing.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lpips_bench needs the GPU: there is nothing to time without it"
    sd = synth.lpips_state_dict(28)
    net = LPIPS()
    net.load_state_dict(sd)
    net = net.cuda()
    tnet = TorchLPIPS(sd)
    lines = []
    for S in a.sizes:
        lines += bench_size(net, tnet, a.batch, S, a.iters)
        print("\n".join(lines[-12:]), flush=True)
    if not a.no_train:
        lines += bench_train(sd, a.batch, a.iters)
    print("\n".join(lines[-4:]))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
