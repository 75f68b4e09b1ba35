"""Generate tests/golden/g21_vq_train.npz from the REAL face-reenactment reference (container only, CPU).

Usage (from the repository root):   python tools/make_golden_vq_train.py

`ldm.models.autoencoder.VQModel.training_step` for optimizer_idx 0 and 1 under `VQLPIPSWithDiscriminator`, with recipe
weights (autoencoder, discriminator and perceptual stand-in alike), for two configurations: `synth.VQ_TRAIN_SMALL` on a 32x32
batch (prefix `a_`) and a narrower one with z_channels = embed_dim = 4, three levels and a 32x48 batch (prefix `b_`).
Three things are arranged at generation time; no reference file is edited:
  * `torchvision.models` exists as an empty stand-in module (taming/modules/losses/lpips.py imports it);
  * ldm/modules/losses/vqperceptual.py uses `exists` without importing it: the reference's own `ldm.util.exists` is bound
    into that module's namespace;
  * `LPIPS()` would download pretrained VGG weights: the name `LPIPS` in that module's namespace is replaced by
    `dsml_thesis_amd.losses.StandInPerceptual`, the module the project's tests inject on their side.
Stored: the state-dict key list with shapes, xrec, idx, every entry of both log dictionaries, (sum, L2 norm) of every
autoencoder parameter gradient, a few gradients in full, the discriminator's gradient norms, and the quantiser statistics
the tests' conditions rest on (smallest best-to-second distance gap, hit histogram).  Arrays and name lists only."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsml_thesis_amd import synth  # noqa: E402
from dsml_thesis_amd.losses import StandInPerceptual  # noqa: E402
from tools.make_golden import load_recipe, rnd, save  # noqa: E402

PERCEPTUAL_SEED = 5
LOSS = dict(disc_start=0, codebook_weight=1.0, disc_num_layers=2, disc_ndf=16, disc_weight=0.8, perceptual_weight=1.0, n_classes=64)
CFG_B = dict(embed_dim=4, n_embed=64,
             ddconfig=dict(double_z=False, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 1, 2],
                           num_res_blocks=1, attn_resolutions=[8], dropout=0.0))
CASES = dict(a=(synth.VQ_TRAIN_SMALL, (2, 32, 32, 3)), b=(CFG_B, (2, 32, 48, 3)))
FULL = ["quantize.embedding.weight", "quant_conv.weight", "quant_conv.bias", "post_quant_conv.weight", "post_quant_conv.bias",
        "encoder.conv_in.weight", "decoder.conv_out.weight", "encoder.down.0.downsample.conv.weight",
        "encoder.mid.attn_1.q.weight", "decoder.norm_out.weight"]


def gen_case(tag, cfg, shape, g):
    from ldm.models.autoencoder import VQModel
    m = VQModel(ddconfig=dict(cfg["ddconfig"]), n_embed=cfg["n_embed"], embed_dim=cfg["embed_dim"],
                lossconfig=dict(target="ldm.modules.losses.vqperceptual.VQLPIPSWithDiscriminator", params=dict(LOSS)))
    load_recipe(m, seed=0)
    m.train()
    m.loss.perceptual_loss.eval()
    m.global_step = 0
    logs = {}
    m.log_dict = lambda d, **kw: logs.update({k: torch.as_tensor(v).detach().clone() for k, v in d.items()})
    sd = m.state_dict()
    g[f"{tag}_keys"] = np.array(list(sd.keys()))
    g[f"{tag}_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    batch = dict(image=torch.tanh(rnd(501, *shape)))
    x = m.get_input(batch, "image")
    with torch.no_grad():
        h = m.encode_to_prequant(x)
        cb = m.quantize.embedding.weight
        zf = h.permute(0, 2, 3, 1).reshape(-1, cb.shape[1])
        d = (zf ** 2).sum(1, keepdim=True) + (cb ** 2).sum(1) - 2 * zf @ cb.t()
        two = d.topk(2, dim=1, largest=False).values
        gap = (two[:, 1] - two[:, 0]).min().item()
    aeloss = m.training_step(batch, 0, 0)
    aeloss.backward()
    xrec, _, ind = m(x, return_pred_indices=True)
    hist = torch.bincount(ind.reshape(-1), minlength=cfg["n_embed"])
    # the tool's own two conditions
    assert gap >= 1e-4, f"[{tag}] smallest best-to-second distance gap {gap:.3e} < 1e-4"
    assert (hist == 0).any() and (hist == 1).any() and (hist > 1).any(), f"[{tag}] hit histogram lacks a 0 / 1 / >1 code"
    g[f"{tag}_gap"], g[f"{tag}_hist"] = np.float64(gap), hist
    g[f"{tag}_xrec"], g[f"{tag}_idx"] = xrec, ind.reshape(-1).to(torch.int32)
    names, stats = [], []
    for k, p in m.named_parameters():
        if k.startswith("loss."):
            continue
        names.append(k)
        stats.append([p.grad.double().sum().item(), p.grad.double().norm().item()])
        if k in FULL:
            g[f"{tag}_grad.{k}"] = p.grad
    g[f"{tag}_grad_names"], g[f"{tag}_grad_stats"] = np.array(names), np.array(stats)
    m.zero_grad()
    discloss = m.training_step(batch, 0, 1)
    discloss.backward()
    dn = [(k, p.grad.double().norm().item()) for k, p in m.loss.discriminator.named_parameters()]
    g[f"{tag}_disc_names"], g[f"{tag}_disc_grad_norms"] = np.array([k for k, _ in dn]), np.array([v for _, v in dn])
    for k, v in logs.items():
        g[f"{tag}_log.{k}"] = v.double()
    print(f"  [{tag}] total {logs['train/total_loss'].item():.6f} quant {logs['train/quant_loss'].item():.6f} "
          f"d_weight {logs['train/d_weight'].item():.6f} gap {gap:.3e} unused/once/more "
          f"{(hist == 0).sum().item()}/{(hist == 1).sum().item()}/{(hist > 1).sum().item()} busiest {hist.max().item()}")


def gen():
    from tools import ref_shims
    ref_shims.install("face_reenactment")
    tv = sys.modules["torchvision"]
    tvm = ref_shims._mod("torchvision.models")
    tv.models = tvm
    import ldm.modules.losses.vqperceptual as vp
    from ldm.util import exists
    vp.exists = exists
    vp.LPIPS = lambda: StandInPerceptual(PERCEPTUAL_SEED)
    g = dict(perceptual_seed=np.int64(PERCEPTUAL_SEED))
    for tag, (cfg, shape) in CASES.items():
        gen_case(tag, cfg, shape, g)
    save("g21_vq_train.npz", **g)


if __name__ == "__main__":
    gen()
