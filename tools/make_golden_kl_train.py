"""Generate tests/golden/g24_kl_train.npz from the REAL face-reenactment reference (container only, CPU).

Usage (from the repository root):   python tools/make_golden_kl_train.py

`ldm.models.autoencoder.AutoencoderKL.training_step` for optimizer_idx 0 and 1 under
`ldm.modules.losses.contperceptual.LPIPSWithDiscriminator`, with recipe weights (autoencoder, discriminator and perceptual
stand-in alike), for two configurations of 32 base channels: two levels with z_channels = embed_dim = 3 on a 32x32 batch
(prefix `a_`: d_weight inside its clamp), and three levels with z_channels = embed_dim = 4 on a 32x48 batch (prefix `b_`:
d_weight on the clamp).
Arranged at generation time; no reference file is edited:
  * `torchvision.models` exists as an empty stand-in module (taming/modules/losses/lpips.py imports it);
  * taming's vqperceptual.py uses `exists` without importing it: the reference's own `ldm.util.exists` is bound in;
  * `LPIPS()` would download pretrained VGG weights: the name `LPIPS` in contperceptual's namespace is replaced by
    `dsml_thesis_amd.losses.StandInPerceptual`, the module the project's tests inject on their side;
  * `DiagonalGaussianDistribution.sample` draws from `torch.randn`: it is wrapped so that each draw's noise is seeded and
    recorded, and the reference's own method, fed that noise, is checked to return mean + std * noise bit for bit.
The tool asserts its own conditions: a's d_weight / disc_weight strictly inside (0, 1e4), b's on the clamp, and every raw
log-variance strictly inside (-30, 20).
Stored per case: the state-dict key list with shapes (`loss.` keys included), both noises, the moments, both draws and
reconstructions, every entry of both log dictionaries, (sum, L2 norm) of every autoencoder parameter gradient, ten gradients
in full, the discriminator's gradient norms -- and the same quantities (suffix `_f64`) from a float64 twin of the reference
(`m.double()`, same inputs, same noise).  Arrays and name lists only."""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsml_thesis_amd.losses import StandInPerceptual  # noqa: E402
from tools.make_golden import load_recipe, rnd, save  # noqa: E402

PERCEPTUAL_SEED = 5
NOISE_SEEDS = (601, 602)            # the draw of optimizer_idx 0, of optimizer_idx 1
LOSS_A = dict(disc_start=0, logvar_init=0.0, kl_weight=1e-6, disc_num_layers=2, disc_weight=0.8, perceptual_weight=1.0)
LOSS_B = dict(LOSS_A, logvar_init=-0.7, kl_weight=0.05)
CFG_A = dict(embed_dim=3,
             ddconfig=dict(double_z=True, z_channels=3, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2],
                           num_res_blocks=1, attn_resolutions=[16], dropout=0.0))
CFG_B = dict(embed_dim=4,
             ddconfig=dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 1, 2],
                           num_res_blocks=1, attn_resolutions=[8], dropout=0.0))
CASES = dict(a=(CFG_A, LOSS_A, (2, 32, 32, 3)), b=(CFG_B, LOSS_B, (2, 32, 48, 3)))
FULL = ["quant_conv.weight", "quant_conv.bias", "post_quant_conv.weight", "post_quant_conv.bias", "encoder.conv_in.weight",
        "encoder.conv_out.weight", "decoder.conv_out.weight", "encoder.down.0.downsample.conv.weight",
        "encoder.mid.attn_1.q.weight", "decoder.norm_out.weight"]


def _seeded_sample(orig, draws, seeds):
    """The wrapper around the reference's DiagonalGaussianDistribution.sample (see the module docstring)."""
    def sample(self):
        noise = rnd(seeds[len(draws) % len(seeds)], *self.mean.shape).to(self.mean.dtype)
        real_randn = torch.randn
        torch.randn = lambda *a, **k: noise
        try:
            x = orig(self)
        finally:
            torch.randn = real_randn
        assert torch.equal(x, self.mean + self.std * noise), "the reference's draw is not mean + std * noise"
        draws.append(dict(noise=noise.detach(), moments=self.parameters.detach(), z=x.detach()))
        return x
    return sample


def run_steps(m, batch, dist_cls):
    """training_step 0 and 1 on `m` -> dict of everything recorded."""
    logs, draws = {}, []
    m.log_dict = lambda d, **kw: logs.update({k: torch.as_tensor(v).detach().clone() for k, v in d.items()})
    orig = dist_cls.sample
    dist_cls.sample = _seeded_sample(orig, draws, NOISE_SEEDS)
    try:
        m.zero_grad()
        aeloss = m.training_step(batch, 0, 0)
        aeloss.backward()
        grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if not k.startswith("loss.")}
        m.zero_grad()
        discloss = m.training_step(batch, 0, 1)
        discloss.backward()
    finally:
        dist_cls.sample = orig
    assert len(draws) == 2
    with torch.no_grad():
        xrec = [m.decode(d["z"]) for d in draws]
    disc = [(k, p.grad.double().norm().item()) for k, p in m.loss.discriminator.named_parameters()]
    return dict(logs=logs, draws=draws, xrec=xrec, grads=grads, disc=disc, aeloss=aeloss.detach(), discloss=discloss.detach())


def gen_case(tag, cfg, loss, shape, g):
    from ldm.models.autoencoder import AutoencoderKL
    from ldm.modules.distributions.distributions import DiagonalGaussianDistribution
    m = AutoencoderKL(ddconfig=dict(cfg["ddconfig"]), embed_dim=cfg["embed_dim"],
                      lossconfig=dict(target="ldm.modules.losses.contperceptual.LPIPSWithDiscriminator", params=dict(loss)))
    load_recipe(m, seed=0)
    m.train()
    m.loss.perceptual_loss.eval()
    m.global_step = 0
    sd = m.state_dict()
    assert "loss.logvar" in sd and float(sd["loss.logvar"]) == np.float32(loss["logvar_init"])
    g[f"{tag}_keys"] = np.array(list(sd.keys()))
    g[f"{tag}_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    twin = copy.deepcopy(m).double()
    twin.get_input = lambda b, k: b[k].permute(0, 3, 1, 2).contiguous().double()       # (the reference's casts to float)
    batch = dict(image=torch.tanh(rnd(501, *shape)))
    for suffix, model in (("", m), ("_f64", twin)):
        r = run_steps(model, batch, DiagonalGaussianDistribution)
        logs, draws = r["logs"], r["draws"]
        raw = draws[0]["moments"][:, cfg["embed_dim"]:]
        if suffix == "":
            dw = logs["train/d_weight"].item() / loss["disc_weight"]
            if tag == "a":
                assert 0.0 < dw < 1e4, f"[a] d_weight / disc_weight = {dw} is not strictly inside (0, 1e4)"
            else:
                assert dw == 1e4, f"[b] d_weight / disc_weight = {dw} is not on the clamp"
            assert -30.0 < raw.min().item() and raw.max().item() < 20.0, f"[{tag}] raw log-variance reaches the clamp"
            assert torch.equal(draws[0]["moments"], draws[1]["moments"]), "the two steps see one set of weights"
            g[f"{tag}_moments"] = draws[0]["moments"]
            g[f"{tag}_noise0"], g[f"{tag}_noise1"] = draws[0]["noise"], draws[1]["noise"]
            g[f"{tag}_grad_names"] = np.array(list(r["grads"]))
            g[f"{tag}_disc_names"] = np.array([k for k, _ in r["disc"]])
            print(f"  [{tag}] total {logs['train/total_loss'].item():.4f} kl {logs['train/kl_loss'].item():.4f} nll "
                  f"{logs['train/nll_loss'].item():.4f} d_weight {logs['train/d_weight'].item():.4f} raw log-variance "
                  f"[{raw.min().item():.3f}, {raw.max().item():.3f}]")
        else:
            assert list(r["grads"]) == g[f"{tag}_grad_names"].tolist()
        for i in (0, 1):
            g[f"{tag}_z{i}{suffix}"], g[f"{tag}_xrec{i}{suffix}"] = draws[i]["z"], r["xrec"][i]
        g[f"{tag}_grad_stats{suffix}"] = np.array([[v.double().sum().item(), v.double().norm().item()] for v in r["grads"].values()])
        for k in FULL:
            g[f"{tag}_grad{suffix}.{k}"] = r["grads"][k]
        g[f"{tag}_disc_grad_norms{suffix}"] = np.array([v for _, v in r["disc"]])
        for k, v in logs.items():
            g[f"{tag}_log{suffix}.{k}"] = v.double()
        assert len(logs) == 11, sorted(logs)


def gen():
    from tools import ref_shims
    ref_shims.install("face_reenactment")
    tv = sys.modules["torchvision"]
    tv.models = ref_shims._mod("torchvision.models")
    import taming.modules.losses.vqperceptual as tvp
    import ldm.modules.losses.vqperceptual as vp
    from ldm.util import exists
    vp.exists = tvp.exists = exists
    import ldm.modules.losses.contperceptual as cp
    cp.LPIPS = lambda: StandInPerceptual(PERCEPTUAL_SEED)
    g = dict(perceptual_seed=np.int64(PERCEPTUAL_SEED))
    for tag, (cfg, loss, shape) in CASES.items():
        gen_case(tag, cfg, loss, shape, g)
    save("g24_kl_train.npz", **g)


if __name__ == "__main__":
    gen()
