"""`LatentDiffusionTune` (talking_face/ldm/models/diffusion/ddpm2condtune.py:447-1112): fine-tune the talking-face UNet, the
class embedder and the audio-window encoder through `q_sample` + 8 differentiable DDIM steps at eta = 1 + the differentiable
first stage, with an image-space lip-reading loss plus a latent l2.

The UNet / decoder forward and backward and the DDIM update run on libldmk kernels (`train.py`, `train_decoder.py`,
`ldmk_ddim_diff_fwd` / `ldmk_ddim_diff_bwd`); the audio-window encoder runs and trains on its fused kernels (`encoders.py`).
The lip-reading network is a pretrained model that is not part of this package: `lip_loss_func(x, x0, landmarks)` is a plain
callable the caller plugs in (the reference's mouth crop + encoder + `1 - mean cosine`, ddpm2condtune.py:1058-1082); a non-zero
`lr_loss_w` without it raises."""
import numpy as np
import torch
import torch.nn.functional as F

from . import train_ops as T
from .ddpm import LatentDiffusion2Cond
from .encoders import audio_attention_backward
from .schedule import ddim_step_table, make_ddim_timesteps
from .train_decoder import DifferentiableDDIM


def adopt_weight(weight, global_step, threshold=20000, value=0.):
    """ddpm2condtune.py:46-49: the loss weight is `value` until `threshold` optimiser steps have been taken."""
    return value if global_step < threshold else weight


class LatentDiffusionTune(LatentDiffusion2Cond):
    def __init__(self, first_stage_config, cond_stage_config_1=None, cond_stage_config_2=None, cond_stage_trainable=True,
                 concat_mode=False, conditioning_key="crossattn", lr_loss_w=1, start_lr_loss=30000, num_tune_steps=8,
                 tune_eta=1.0, **kwargs):
        assert conditioning_key in ["crossattn"]                                   # ddpm2condtune.py:469-471
        assert cond_stage_trainable is True
        assert concat_mode is False
        super().__init__(first_stage_config, cond_stage_config_1, cond_stage_config_2, cond_stage_trainable=cond_stage_trainable,
                         concat_mode=concat_mode, conditioning_key=conditioning_key, **kwargs)
        from .sampling_loop import require_eps_model
        require_eps_model(self, type(self).__name__)
        from .autoencoder import VQModelInterface
        if not isinstance(self.first_stage_model, VQModelInterface):
            raise NotImplementedError(f"{type(self).__name__}: the fine-tune decodes differentiably through a VQ first stage; "
                                      f"{type(self.first_stage_model).__name__} is not built for it")
        self.lr_loss_w, self.start_lr_loss = lr_loss_w, start_lr_loss
        self.lip_loss_func = None                                                   # plugged in by the caller
        self.num_tune_steps, self.tune_eta = num_tune_steps, tune_eta               # make_schedule(8, ddim_eta=1.0), :533
        self._ddd = self._tune_table = None

    def tune_table(self):
        """(timesteps, [S][4] coefficient rows) of the fine-tune walk, built on the host once."""
        if self._tune_table is None:
            ts = make_ddim_timesteps("uniform", self.num_tune_steps, self.num_timesteps)
            self._tune_table = (np.asarray(ts), ddim_step_table(self.alphas_cumprod.detach().cpu(), ts, self.tune_eta))
        return self._tune_table

    def differentiable(self):
        if self._ddd is None:
            self._ddd = DifferentiableDDIM(self)
        return self._ddd

    def tune_losses(self, x, x0, z, z0, l):
        """ddpm2condtune.py:1054-1112 on the decoded images (x: requires_grad leaf, x0: decode of the clean latent), the walk's
        final latent z (leaf) and the clean latent z0."""
        prefix = "train" if self.training else "val"
        x, x0 = torch.clamp(x, min=-1.0, max=1.0), torch.clamp(x0, min=-1.0, max=1.0)
        loss_dict = {}
        lr_loss = x.new_zeros(())
        if self.lr_loss_w:
            lr_loss = self.lip_loss_func(x, x0, l)
            loss_dict[f"{prefix}_lr_loss"] = lr_loss
        l2_loss = F.mse_loss(z, z0)
        loss_dict[f"{prefix}_l2_loss"] = l2_loss
        loss = adopt_weight(self.lr_loss_w, self.trainer().P.step, threshold=self.start_lr_loss) * lr_loss + l2_loss
        loss_dict[f"{prefix}_loss"] = loss
        return loss, loss_dict

    def forward(self, x, c1, c2, c3, c4, l, t=None, noise=None, ddim_noise=None):
        """ddpm2condtune.py:947-960 + p_losses: x = clean latents, c1 = the batch holding the class labels, c2 = (b,T,768)
        audio window, c3 / c4 = masked-frame / identity latents, l = landmarks (handed to `lip_loss_func`).  t, the q_sample
        noise and the S draws of the DDIM steps are drawn unless given.  Leaves the gradients of the UNet in
        `self.trainer().P.grad` and those of the two conditioners in their parameters' `.grad`.  Returns (loss, loss_dict)."""
        assert c1 is not None and c2 is not None
        if self.lr_loss_w and self.lip_loss_func is None:
            raise NotImplementedError("LatentDiffusionTune: lr_loss_w != 0 needs a `lip_loss_func` callable "
                                      "(the pretrained lip-reading network is not part of this package)")
        dev = x.device
        x = x.float().contiguous()
        t = torch.randint(0, self.num_timesteps, (x.shape[0],), device=dev).long() if t is None else t
        with torch.enable_grad():
            c1e = self.cond_stage_model_1(c1, training=self.training)      # ddpm2condtune.py:613
        c2 = c2.float().contiguous()
        c2e = self.cond_stage_model_2(c2)
        assert c1e.dim() == 3 and c2e.dim() == 3
        c12 = torch.cat([c1e.detach().float(), c2e], dim=2)
        c34 = torch.cat([c3, c4], dim=1).float()
        noise = torch.randn_like(x) if noise is None else noise.float().contiguous()
        x_noisy = T.q_sample(x, noise, t, self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod)
        ts, table = self.tune_table()
        dd = self.differentiable()
        img = dd.forward(x_noisy, c12, table, ts, noise=ddim_noise, c_concat=c34)
        img0 = self.decode_first_stage(x)
        with torch.enable_grad():
            leaf, zleaf = img.detach().requires_grad_(True), dd.z.detach().requires_grad_(True)
            loss, loss_dict = self.tune_losses(leaf, img0, zleaf, x, l)
            loss.backward()
        dd.backward(torch.zeros_like(img) if leaf.grad is None else leaf.grad, dz=zleaf.grad)
        d12 = dd.d_context
        for m in (self.cond_stage_model_1, self.cond_stage_model_2):
            for p_ in m.parameters():
                p_.grad = None
        n1 = c1e.shape[2]
        if c1e.requires_grad:
            c1e.backward(d12[..., :n1].contiguous().to(c1e.dtype))
        audio_attention_backward(self.cond_stage_model_2, c2, d12[..., n1:].contiguous())
        return loss.detach(), {k: v.detach() for k, v in loss_dict.items()}

    def training_step_latents(self, x, c1, c2, c3, c4, l, lr, t=None, noise=None, ddim_noise=None, world_size=1,
                              weight_decay=1e-2):
        """One fine-tune step on encoded latents (ddpm2condtune.py shared_step -> forward -> p_losses): AdamW on the UNet
        (ldmk_adamw over the flat buffer) and on the two conditioners (torch), then the EMA update."""
        tr = self.trainer()
        loss, loss_dict = self(x, c1, c2, c3, c4, l, t=t, noise=noise, ddim_noise=ddim_noise)
        if world_size > 1:
            tr.all_reduce_grads(world_size)
        tr.adamw_step(lr, weight_decay=weight_decay)
        for key, owner in (("_cond_opt", self.cond_stage_model_1), ("_audio_opt", self.cond_stage_model_2)):
            if getattr(self, key, None) is None:
                setattr(self, key, torch.optim.AdamW(owner.parameters(), lr=lr, weight_decay=weight_decay))
            opt = getattr(self, key)
            for grp in opt.param_groups:
                grp["lr"] = lr
            opt.step()
        if self.use_ema:
            decay = float(self.model_ema.decay)
            if int(self.model_ema.num_updates) >= 0:
                self.model_ema.num_updates += 1
                n_up = int(self.model_ema.num_updates)
                decay = min(decay, (1 + n_up) / (10 + n_up))
            tr.ema_update(self._ema_flat, decay)
        return loss, loss_dict
