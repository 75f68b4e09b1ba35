"""The first-stage training losses: the VQGAN's (ldm/modules/losses/vqperceptual.py:43-167) and the KL autoencoder's
(ldm/modules/losses/contperceptual.py:7-110); the PatchGAN of both (taming/modules/discriminator/model.py:17-67).

`VQLPIPSWithDiscriminator` turns a reconstruction into the image gradient `FirstStageTrainer.backward` takes.  The pixel
term runs on ldmk_l1_grad / ldmk_mse_grad; the PatchGAN discriminator is a plain torch module on PyTorch-ROCm autograd, the
arrangement the CLIP / ArcFace losses of the fine-tuning models have.  The perceptual network is injected: pretrained LPIPS
weights cannot be obtained offline, so `perceptual_weight > 0` without a module is refused.  `dsml_thesis_amd.lpips.LPIPS` is
the real one (VGG16, value and image gradient on HIP, weights from local files; DESIGN §25 has its cost: 3 % of a KL-f4
step); `StandInPerceptual` below is what the fixtures inject, and only of that stand-in is it true that the perceptual
term is well under 1 % of the step.

One backward per autoencoder step:
    loss    = nll + d_weight * disc_factor * g + codebook_weight * qloss,   nll = mean(pixel + perceptual_weight * p)
    d_image = d nll / d xrec + d_weight * disc_factor * d g / d xrec
    d_weight = clamp(|d nll / d W_last| / (|d g / d W_last| + 1e-4), 0, 1e4) * disc_weight
where the two last-layer gradients come from `last_layer(d_image_term)` -- `FirstStageTrainer.last_layer_grad`.

`LPIPSWithDiscriminator` is the same arrangement for `AutoencoderKL`: the pixel term is a sum under a learned-scale NLL
(ldmk_l1_sum_grad), and the KL term enters at the bottleneck (`FirstStageTrainer.backward(kl_weight=...)`), not here."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import train_ops as T


def adopt_weight(weight, global_step, threshold=0, value=0.0):
    return value if global_step < threshold else weight


def hinge_d_loss(logits_real, logits_fake):
    return 0.5 * (F.relu(1.0 - logits_real).mean() + F.relu(1.0 + logits_fake).mean())


def vanilla_d_loss(logits_real, logits_fake):
    return 0.5 * (F.softplus(-logits_real).mean() + F.softplus(logits_fake).mean())


def perplexity_from_counts(counts):
    """(perplexity, cluster_usage) of the code histogram, vqperceptual.py:26-33: exp(-sum p log(p + 1e-10)), #(p > 0)."""
    p = counts.float() / counts.sum().float()
    return torch.exp(-(p * torch.log(p + 1e-10)).sum()), (p > 0).sum()


class NLayerDiscriminator(nn.Module):
    """PatchGAN: 4x4 convolutions, stride 2 for the first n_layers, BatchNorm from the second on, LeakyReLU(0.2), a one-channel
    logit map.  State-dict keys `main.N.*` with the reference's indices."""

    def __init__(self, input_nc=3, ndf=64, n_layers=3, use_actnorm=False):
        super().__init__()
        if use_actnorm:
            raise NotImplementedError("NLayerDiscriminator: use_actnorm is not built (BatchNorm only)")
        seq = [nn.Conv2d(input_nc, ndf, 4, 2, 1), nn.LeakyReLU(0.2, True)]
        mult = 1
        for n in range(1, n_layers + 1):
            prev, mult = mult, min(2 ** n, 8)
            seq += [nn.Conv2d(ndf * prev, ndf * mult, 4, 2 if n < n_layers else 1, 1, bias=False), nn.BatchNorm2d(ndf * mult),
                    nn.LeakyReLU(0.2, True)]
        seq.append(nn.Conv2d(ndf * mult, 1, 4, 1, 1))
        self.main = nn.Sequential(*seq)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0.0, 0.02)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.normal_(m.weight, 1.0, 0.02)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        return self.main(x)


class VQLPIPSWithDiscriminator(nn.Module):
    def __init__(self, disc_start, codebook_weight=1.0, pixelloss_weight=1.0, disc_num_layers=3, disc_in_channels=3,
                 disc_factor=1.0, disc_weight=1.0, perceptual_weight=1.0, use_actnorm=False, disc_conditional=False, disc_ndf=64,
                 disc_loss="hinge", n_classes=None, perceptual_loss="lpips", pixel_loss="l1"):
        super().__init__()
        if disc_loss not in ("hinge", "vanilla") or pixel_loss not in ("l1", "l2"):
            raise ValueError(f"VQLPIPSWithDiscriminator: disc_loss={disc_loss!r}, pixel_loss={pixel_loss!r}")
        if use_actnorm or disc_conditional:
            raise NotImplementedError("VQLPIPSWithDiscriminator: use_actnorm / disc_conditional are not built")
        self.perceptual_loss = _perceptual_module("VQLPIPSWithDiscriminator", perceptual_loss, perceptual_weight)
        self.codebook_weight, self.pixel_weight, self.perceptual_weight = codebook_weight, pixelloss_weight, perceptual_weight
        self.pixel_loss = pixel_loss
        self.discriminator = NLayerDiscriminator(input_nc=disc_in_channels, n_layers=disc_num_layers, ndf=disc_ndf)
        self.discriminator_iter_start = disc_start
        self.disc_loss = hinge_d_loss if disc_loss == "hinge" else vanilla_d_loss
        self.disc_factor, self.discriminator_weight, self.n_classes = disc_factor, disc_weight, n_classes
        self.d_image = None

    def calculate_adaptive_weight(self, nll_last, g_last):
        """The two arguments are the last layer's weight gradients of the nll and of the generator term."""
        d_weight = torch.norm(nll_last) / (torch.norm(g_last) + 1e-4)
        return torch.clamp(d_weight, 0.0, 1e4).detach() * self.discriminator_weight

    def forward(self, codebook_loss, inputs, reconstructions, optimizer_idx, global_step, last_layer=None, cond=None,
                split="train", predicted_indices=None, counts=None):
        """The reference's signature.  optimizer_idx 0 -> (loss, log) and `self.d_image`, the gradient of everything but the
        codebook term with respect to the reconstruction; `last_layer` is a callable image gradient -> last-layer weight
        gradient (None: d_weight = 0, as the reference has it outside training).  optimizer_idx 1 -> (d_loss, log) with
        autograd attached to the discriminator's parameters.  `counts` (hits per code) or `predicted_indices` give the
        perplexity entries."""
        if cond is not None:
            raise NotImplementedError("VQLPIPSWithDiscriminator: disc_conditional is not built")
        x, xrec = inputs.contiguous().float(), reconstructions.detach().contiguous().float()
        disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
        if optimizer_idx == 1:
            logits_real, logits_fake = self.discriminator(x), self.discriminator(xrec)
            d_loss = disc_factor * self.disc_loss(logits_real, logits_fake)
            return d_loss, {f"{split}/disc_loss": d_loss.detach().mean(), f"{split}/logits_real": logits_real.detach().mean(),
                            f"{split}/logits_fake": logits_fake.detach().mean()}
        if codebook_loss is None:
            codebook_loss = torch.zeros(1, device=x.device)
        pix, d_nll = (T.l1_grad if self.pixel_loss == "l1" else T.mse_grad)(xrec, x)
        rec_mean, p_mean = pix[0], torch.zeros((), device=x.device)
        leaf = xrec.clone().requires_grad_(True)
        with torch.enable_grad():
            if self.perceptual_loss is not None and self.perceptual_weight > 0:
                p = self.perceptual_loss(x, leaf).mean()
                p_mean = p.detach()
                d_nll = d_nll + self.perceptual_weight * torch.autograd.grad(p, leaf)[0]
            g_loss = -self.discriminator(leaf).mean()
            d_g = torch.autograd.grad(g_loss, leaf)[0]
        nll = rec_mean + self.perceptual_weight * p_mean
        if last_layer is not None:
            d_weight = self.calculate_adaptive_weight(last_layer(d_nll), last_layer(d_g))
        else:
            d_weight = torch.zeros((), device=x.device)
        g_loss = g_loss.detach()
        self.d_image = d_nll + (d_weight * disc_factor) * d_g
        loss = nll + d_weight * disc_factor * g_loss + self.codebook_weight * codebook_loss.mean()
        log = {f"{split}/total_loss": loss.detach().mean(), f"{split}/quant_loss": codebook_loss.detach().mean(),
               f"{split}/nll_loss": nll.detach(), f"{split}/rec_loss": nll.detach(), f"{split}/p_loss": p_mean,
               f"{split}/d_weight": d_weight.detach(), f"{split}/disc_factor": torch.tensor(disc_factor),
               f"{split}/g_loss": g_loss}
        if counts is None and predicted_indices is not None:
            counts = torch.bincount(predicted_indices.reshape(-1).long(), minlength=self.n_classes)
        if counts is not None:
            log[f"{split}/perplexity"], log[f"{split}/cluster_usage"] = perplexity_from_counts(counts)
        return loss, log


def _perceptual_module(name, perceptual_loss, perceptual_weight):
    """The injected perceptual network of both losses: a module, a `target` dict naming one, or nothing with weight 0."""
    if isinstance(perceptual_loss, dict) and "target" in perceptual_loss:      # a YAML lossconfig names the network
        from .util import instantiate_from_config
        perceptual_loss = instantiate_from_config(perceptual_loss)
    if isinstance(perceptual_loss, nn.Module):
        return perceptual_loss.eval()
    if perceptual_weight > 0:
        raise NotImplementedError(f"{name}: perceptual_weight > 0 needs a perceptual network, and the "
                                  "pretrained LPIPS weights cannot be obtained offline: pass one as perceptual_loss=<module> "
                                  "(inputs, reconstructions) -> (n,1,1,1) -- dsml_thesis_amd.lpips.LPIPS(vgg_ckpt=..., lpips_ckpt=...) "
                                  "is LPIPS on HIP from local weight files, also as perceptual_loss={target: "
                                  "taming.modules.losses.lpips.LPIPS, params: {vgg_ckpt: ..., lpips_ckpt: ...}} -- or set "
                                  "perceptual_weight=0")
    return None


class LPIPSWithDiscriminator(nn.Module):
    """contperceptual.py:7-110, the loss of AutoencoderKL.  With C*H*W the image size per sample and n the batch:
        rec_sum  = sum|x - xrec| + perceptual_weight * C*H*W * sum_b p_b
        nll      = rec_sum / (exp(logvar) * n) + logvar * C*H*W
        kl_loss  = sum_b kl_b / n
        loss     = nll + kl_weight * kl_loss + d_weight * disc_factor * g_loss
        d_image  = d nll / d xrec + d_weight * disc_factor * d g_loss / d xrec          (the KL term has no image gradient)
    `logvar` is an nn.Parameter stored under `loss.logvar`, as in the reference; no optimizer of the reference owns it
    (autoencoder.py:386-395), so it never moves, and its gradient is NOT computed here.  The perceptual network is injected
    (`perceptual_loss=<module>`), as for VQLPIPSWithDiscriminator."""

    def __init__(self, disc_start, logvar_init=0.0, kl_weight=1.0, pixelloss_weight=1.0, disc_num_layers=3, disc_in_channels=3,
                 disc_factor=1.0, disc_weight=1.0, perceptual_weight=1.0, use_actnorm=False, disc_conditional=False,
                 disc_loss="hinge", perceptual_loss="lpips"):
        super().__init__()
        if disc_loss not in ("hinge", "vanilla"):
            raise ValueError(f"LPIPSWithDiscriminator: disc_loss={disc_loss!r}")
        if use_actnorm or disc_conditional:
            raise NotImplementedError("LPIPSWithDiscriminator: use_actnorm / disc_conditional are not built")
        self.perceptual_loss = _perceptual_module("LPIPSWithDiscriminator", perceptual_loss, perceptual_weight)
        self.kl_weight, self.pixel_weight, self.perceptual_weight = kl_weight, pixelloss_weight, perceptual_weight
        self.logvar = nn.Parameter(torch.ones(size=()) * logvar_init)
        self.discriminator = NLayerDiscriminator(input_nc=disc_in_channels, n_layers=disc_num_layers)
        self.discriminator_iter_start = disc_start
        self.disc_loss = hinge_d_loss if disc_loss == "hinge" else vanilla_d_loss
        self.disc_factor, self.discriminator_weight, self.disc_conditional = disc_factor, disc_weight, disc_conditional
        self.d_image = None
        self._lv = None

    calculate_adaptive_weight = VQLPIPSWithDiscriminator.calculate_adaptive_weight

    def _logvar_host(self):
        """(logvar, exp(logvar)) as Python floats, read from the device again only when the parameter has changed."""
        key = (self.logvar.data_ptr(), self.logvar._version)
        if self._lv is None or self._lv[0] != key:
            lv = float(self.logvar.detach())
            self._lv = (key, lv, math.exp(lv))
        return self._lv[1], self._lv[2]

    def assemble(self, rec_sum, p_sum, kl, g_loss, d_weight, disc_factor, n, chw, split="train"):
        """The host arithmetic of the generator step from its ingredients (tensors on any device): -> (loss, log) with the
        reference's eight log entries (contperceptual.py:85-91)."""
        lv = self.logvar.detach().to(rec_sum.device)
        rec_total = rec_sum + self.perceptual_weight * chw * p_sum
        nll = rec_total / (torch.exp(lv) * n) + lv * chw
        kl_loss = kl.sum() / kl.shape[0]
        loss = nll + self.kl_weight * kl_loss + d_weight * disc_factor * g_loss
        log = {f"{split}/total_loss": loss.detach().mean(), f"{split}/logvar": self.logvar.detach(),
               f"{split}/kl_loss": kl_loss.detach().mean(), f"{split}/nll_loss": nll.detach().mean(),
               f"{split}/rec_loss": (rec_total / (n * chw)).detach().mean(), f"{split}/d_weight": d_weight.detach(),
               f"{split}/disc_factor": torch.tensor(disc_factor), f"{split}/g_loss": g_loss.detach().mean()}
        return loss, log

    def forward(self, inputs, reconstructions, posteriors, optimizer_idx, global_step, last_layer=None, cond=None,
                split="train", weights=None):
        """The reference's signature.  `posteriors`: a DiagonalGaussianDistribution, or the per-sample KL (n,) the trainer's
        forward kept.  optimizer_idx 0 -> (loss, log) and `self.d_image` for `FirstStageTrainer.backward`; `last_layer` is a
        callable image gradient -> last-layer weight gradient (None: d_weight = 0).  optimizer_idx 1 -> (d_loss, log) with
        autograd attached to the discriminator's parameters."""
        if cond is not None or weights is not None:
            raise NotImplementedError("LPIPSWithDiscriminator: cond (disc_conditional) and weights are not built")
        x, xrec = inputs.contiguous().float(), reconstructions.detach().contiguous().float()
        disc_factor = adopt_weight(self.disc_factor, global_step, threshold=self.discriminator_iter_start)
        if optimizer_idx == 1:
            logits_real, logits_fake = self.discriminator(x), self.discriminator(xrec)
            d_loss = disc_factor * self.disc_loss(logits_real, logits_fake)
            return d_loss, {f"{split}/disc_loss": d_loss.detach().mean(), f"{split}/logits_real": logits_real.detach().mean(),
                            f"{split}/logits_fake": logits_fake.detach().mean()}
        n, chw = x.shape[0], x[0].numel()
        kl = posteriors if torch.is_tensor(posteriors) else posteriors.kl()
        _, var = self._logvar_host()
        scale = 1.0 / (var * n)                                     # d nll / d rec_sum
        rec_sum, d_nll = T.l1_sum_grad(xrec, x, scale)
        rec_sum, p_sum = rec_sum[0], torch.zeros((), device=x.device)
        leaf = xrec.clone().requires_grad_(True)
        with torch.enable_grad():
            if self.perceptual_loss is not None and self.perceptual_weight > 0:
                p = self.perceptual_loss(x, leaf).sum()
                p_sum = p.detach()
                d_nll = d_nll + (self.perceptual_weight * chw * scale) * torch.autograd.grad(p, leaf)[0]
            g_loss = -self.discriminator(leaf).mean()
            d_g = torch.autograd.grad(g_loss, leaf)[0]
        if last_layer is not None and self.disc_factor > 0.0:
            d_weight = self.calculate_adaptive_weight(last_layer(d_nll), last_layer(d_g))
        else:
            d_weight = torch.zeros((), device=x.device)
        self.d_image = d_nll + (d_weight * disc_factor) * d_g
        return self.assemble(rec_sum, p_sum, kl.to(x.device), g_loss.detach(), d_weight, disc_factor, n, chw, split)


class StandInPerceptual(nn.Module):
    """A small seeded feature-distance network with the call shape of LPIPS, (inputs, reconstructions) -> (n,1,1,1): what
    tests and fixtures inject where the pretrained VGG weights of LPIPS cannot be had.  It measures nothing perceptual."""

    def __init__(self, seed=0, width=8):
        super().__init__()
        self.seed = seed
        self.c1, self.c2 = nn.Conv2d(3, width, 3, 2, 1), nn.Conv2d(width, width, 3, 1, 1)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.02))

    def features(self, x):
        f1 = torch.tanh(self.c1(x))
        return f1, torch.tanh(self.c2(f1))

    def forward(self, inputs, reconstructions):
        return sum(((a - b) ** 2).mean(dim=(1, 2, 3), keepdim=True)
                   for a, b in zip(self.features(inputs), self.features(reconstructions)))
