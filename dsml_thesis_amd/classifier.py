"""NoisyLatentImageClassifier: drop-in for the `pl.LightningModule` of the reference
(face_reenactment/ldm/models/diffusion/classifier.py:28-268), and ClassifierGuidance, the `score_corrector` made of it.

The classifier is an `EncoderUNetModel` built from the diffusion UNet's own params (`load_classifier`, classifier.py:95-102) and
trained on noisy latents `q_sample(x0, t)` against the class label, with F.cross_entropy.  Forward, backward and AdamW run on the
HIP training engine (train.EncoderUNetTrainer); `training_step` leaves the gradients in `trainer().P.grad`, `train_batch` is
step + AdamW, as on the other trainable models here.  Inference (`forward`, `validation_step`) is the trainer's forward with the tape
dropped.

Where this differs from the reference, on purpose:
  * `get_x_noisy` of the reference reads `diffusion_model.use_continuous_noise` and passes `continuous_sqrt_alpha_cumprod=` to
    `q_sample` (classifier.py:110-118); no diffusion model of the reference has either, so its `shared_step` raises on its own models.
    Here `getattr(diffusion_model, "use_continuous_noise", False)` is read: false runs the discrete `q_sample`, true raises
    NotImplementedError.
  * `label_key == 'segmentation'` (a full UNetModel with per-pixel cross-entropy) and `log_images` are not built.
  * `diffusion_model=` injects a built, frozen model in place of the `diffusion_path` glob.
"""
import glob
import os
import re
from copy import deepcopy

import torch

from . import train_ops as T
from .ddpm import _Base
from .encoder_unet import EncoderUNetModel
from .util import instantiate_from_config, load_yaml_config

__models__ = {"class_label": EncoderUNetModel}           # classifier.py:16-19; 'segmentation' -> UNetModel is not built

_UNET_KWARGS = ("image_size", "in_channels", "model_channels", "out_channels", "num_res_blocks", "attention_resolutions", "dropout",
                "channel_mult", "conv_resample", "num_classes", "use_checkpoint", "num_heads", "num_head_channels",
                "num_heads_upsample", "use_scale_shift_norm", "resblock_updown", "use_new_attention_order",
                "use_spatial_transformer", "transformer_depth", "context_dim")


def unet_params_of(unet):
    """The constructor kwargs of a built UNetModel (what `diffusion_config.params.unet_config.params` holds in the reference)."""
    return {k: deepcopy(getattr(unet, k)) for k in _UNET_KWARGS if hasattr(unet, k)}


def classifier_config(unet_params, num_classes, pool, label_key="class_label"):
    """classifier.py:95-102: a deep copy of the diffusion UNet's params with in_channels <- the UNet's out_channels,
    out_channels <- num_classes and, for 'class_label', pool <- pool."""
    cfg = deepcopy(dict(unet_params))
    cfg["in_channels"] = unet_params["out_channels"]
    cfg["out_channels"] = num_classes
    if label_key == "class_label":
        cfg["pool"] = pool
    return cfg


def _natural(s):
    return [int(p) if p.isdigit() else p for p in re.split(r"(\d+)", s)]


class _AdamWOfTrainer:
    """What configure_optimizers hands out: the step is ldmk_adamw over the trainer's flat buffer."""

    def __init__(self, model, lr, weight_decay):
        self.model = model
        self.param_groups = [dict(lr=lr, weight_decay=weight_decay)]

    def step(self):
        g = self.param_groups[0]
        self.model.trainer().adamw_step(g["lr"], weight_decay=g["weight_decay"])
        self.model._dirty = True

    def zero_grad(self, set_to_none=False):
        self.model.trainer().P.grad.zero_()


class NoisyLatentImageClassifier(_Base):
    def __init__(self, diffusion_path=None, num_classes=None, ckpt_path=None, pool="attention", label_key=None,
                 diffusion_ckpt_path=None, scheduler_config=None, weight_decay=1.e-2, log_steps=10, monitor="val/loss",
                 diffusion_model=None, compute="f32", *args, **kwargs):
        super().__init__()
        assert num_classes is not None, "num_classes is required"
        self.num_classes = num_classes
        if diffusion_model is not None:
            object.__setattr__(self, "diffusion_model", None)
            self.diffusion_config = None
            self._unet_params = unet_params_of(diffusion_model.model.diffusion_model)
        else:
            # the latest config of the diffusion model's log directory (classifier.py:45-48)
            found = sorted(glob.glob(os.path.join(diffusion_path, "configs", "*-project.yaml")), key=_natural)
            if not found:
                raise FileNotFoundError(f"no configs/*-project.yaml under {diffusion_path}")
            self.diffusion_config = load_yaml_config(found[-1])["model"]
            self.diffusion_config["params"]["ckpt_path"] = diffusion_ckpt_path
            self._unet_params = dict(self.diffusion_config["params"]["unet_config"]["params"])
        self.load_diffusion(diffusion_model)
        self.monitor = monitor
        enc = getattr(getattr(self.diffusion_model, "first_stage_model", None), "encoder", None)
        self.numd = getattr(enc, "num_resolutions", 1) - 1
        self.log_time_interval = self.diffusion_model.num_timesteps // log_steps
        self.log_steps = log_steps
        self.label_key = label_key if not hasattr(self.diffusion_model, "cond_stage_key") else self.diffusion_model.cond_stage_key
        assert self.label_key is not None, "label_key neither in diffusion model nor in model.params"
        if self.label_key not in __models__:
            raise NotImplementedError(f"NoisyLatentImageClassifier: label_key '{self.label_key}' (built: 'class_label'; "
                                      "'segmentation', a full UNetModel with per-pixel cross-entropy, is not)")
        self.compute = compute
        self._tr, self._guide, self._guide_step, self._dirty, self._opt = None, None, -1, False, None
        self.learning_rate, self.global_step, self.logged = 1e-4, 0, {}
        self.load_classifier(ckpt_path, pool)
        self.scheduler_config = scheduler_config
        self.use_scheduler = self.scheduler_config is not None
        self.weight_decay = weight_decay
        self.lr_schedule = None
        self.reset_noise_accs()

    # ---- construction ------------------------------------------------------------------------------------
    def init_from_ckpt(self, path, ignore_keys=list(), only_model=False):
        sd = torch.load(path, map_location="cpu")
        if "state_dict" in list(sd.keys()):
            sd = sd["state_dict"]
        for k in list(sd.keys()):
            for ik in ignore_keys:
                if k.startswith(ik):
                    print("Deleting key {} from state_dict.".format(k))
                    del sd[k]
        target = self.model if only_model else self
        missing, unexpected = target.load_state_dict(sd, strict=False)
        self._tr = self._guide = None
        print(f"Restored from {path} with {len(missing)} missing and {len(unexpected)} unexpected keys")
        return missing, unexpected

    def load_diffusion(self, model=None):
        model = instantiate_from_config(self.diffusion_config) if model is None else model
        model = model.eval()
        for param in model.parameters():
            param.requires_grad = False
        # frozen and kept out of the module tree: the classifier's parameters / state dict are its own network's (the reference
        # registers the diffusion model as a child and freezes it, classifier.py:88-93)
        object.__setattr__(self, "diffusion_model", model)

    def load_classifier(self, ckpt_path, pool):
        self.model_config = classifier_config(self._unet_params, self.num_classes, pool, self.label_key)
        self.model = __models__[self.label_key](**self.model_config)
        if ckpt_path is not None:
            print(f'load from ckpt "{ckpt_path}"')
            self.init_from_ckpt(ckpt_path)

    # ---- the HIP training engine ----------------------------------------------------------------------------
    def trainer(self):
        if self._tr is None:
            from .train import EncoderUNetTrainer
            self.model.pack_weights()
            self._tr = EncoderUNetTrainer(self.model, compute=self.compute)
        return self._tr

    def _guidance_trainer(self):
        """The trainer log_prob_grad runs on: one of its own (want_dx, its own tape and gradient buffer), so the parameter gradients
        a guidance pass computes as a by-product never touch a training step in flight.  Its weights follow the training
        trainer's (one device copy of the flat buffer after an optimizer step)."""
        if self._guide is None:
            from .train import EncoderUNetTrainer
            self.sync_trained_weights()
            self.model.pack_weights()
            self._guide = EncoderUNetTrainer(self.model, compute=self.compute, want_dx=True)
            self._guide_step = -1 if self._tr is None else self._tr.P.step
        if self._tr is not None and self._tr.P.step != self._guide_step:
            self._guide.P.flat.copy_(self._tr.P.flat)
            self._guide_step = self._tr.P.step
        return self._guide

    def sync_trained_weights(self):
        """Write the trained (flat, packed) weights back into the module's nn.Parameters."""
        if self._dirty and self._tr is not None:
            self._tr.sync_to_module()
            self._dirty = False

    def state_dict(self, *args, **kwargs):
        self.sync_trained_weights()
        return super().state_dict(*args, **kwargs)

    # ---- the reference's surface ----------------------------------------------------------------------------
    @torch.no_grad()
    def get_x_noisy(self, x, t, noise=None):
        if getattr(self.diffusion_model, "use_continuous_noise", False):
            raise NotImplementedError("NoisyLatentImageClassifier: use_continuous_noise (no diffusion model of the reference has "
                                      "sample_continuous_noise_level; only the discrete q_sample is built)")
        dm = self.diffusion_model
        noise = torch.randn_like(x) if noise is None else noise
        return T.q_sample(x.contiguous().float(), noise.contiguous().float(), t.to(torch.int64).contiguous(),
                          dm.sqrt_alphas_cumprod.to(x.device).contiguous(), dm.sqrt_one_minus_alphas_cumprod.to(x.device).contiguous())

    def forward(self, x_noisy, t, *args, **kwargs):
        if self._tr is not None:
            return self._tr.forward(x_noisy, t, keep_tape=False)
        return self.model(x_noisy, t)

    @torch.no_grad()
    def get_input(self, batch, k):
        x = batch[k]
        if len(x.shape) == 3:
            x = x[..., None]
        return x.permute(0, 3, 1, 2).to(memory_format=torch.contiguous_format).float()

    @torch.no_grad()
    def get_conditioning(self, batch, k=None):
        if k is None:
            k = self.label_key
        assert k is not None, "Needs to provide label key"
        return torch.as_tensor(batch[k]).to(self.device)

    def compute_top_k(self, logits, labels, k, reduction="mean"):
        _, top_ks = torch.topk(logits, k, dim=1)
        if reduction == "mean":
            return (top_ks == labels[:, None]).float().sum(dim=-1).mean().item()
        elif reduction == "none":
            return (top_ks == labels[:, None]).float().sum(dim=-1)

    @torch.no_grad()
    def write_logs(self, loss, logits, targets):
        log_prefix = "train" if self.training else "val"
        log = {f"{log_prefix}/loss": loss.mean(),
               f"{log_prefix}/acc@1": self.compute_top_k(logits, targets, k=1, reduction="mean"),
               f"{log_prefix}/acc@5": self.compute_top_k(logits, targets, k=min(5, logits.shape[1]), reduction="mean")}
        self.logged.update(log)
        try:
            self.log_dict(log, prog_bar=False, logger=True, on_step=self.training, on_epoch=True)
        except Exception:                      # outside a Lightning loop there is nobody to log to
            pass

    def shared_step(self, batch, t=None, backward=None):
        """classifier.py:179-196 -> (loss, logits, x_noisy, targets).  `backward` (default: the module is in training mode): the
        pass keeps its tape and the gradient of the mean loss is left in trainer().P.grad; else it is a forward only.  The
        per-sample losses (reduction='none') stay in `self.loss_per`."""
        x, *_ = self.diffusion_model.get_input(batch, k=self.diffusion_model.first_stage_key)
        targets = self.get_conditioning(batch)
        if targets.dim() == 4:
            targets = targets.argmax(dim=1)
        dev = x.device
        if t is None:
            t = torch.randint(0, self.diffusion_model.num_timesteps, (x.shape[0],), device=dev).long()
        elif not torch.is_tensor(t):
            t = torch.full(size=(x.shape[0],), fill_value=int(t), device=dev).long()
        return self.step_latents(x, targets.to(dev), t, backward=backward)

    def step_latents(self, x, targets, t, noise=None, backward=None):
        """`shared_step` on already-encoded latents x with given timesteps (and, optionally, the noise of q_sample)."""
        backward = self.training if backward is None else backward
        x_noisy = self.get_x_noisy(x, t, noise)
        targets = targets.to(torch.int64).contiguous()
        tr = self.trainer()
        logits = tr.forward(x_noisy, t, keep_tape=bool(backward))
        per, mean, dl = T.cross_entropy(logits, targets, want_dlogits=bool(backward))
        if backward:
            tr.backward(dl)
        self.loss_per = per
        self.write_logs(per.detach(), logits.detach(), targets.detach())
        return mean[0], logits, x_noisy, targets

    def training_step(self, batch, batch_idx=0):
        loss, *_ = self.shared_step(batch, backward=True)
        return loss

    def train_batch(self, batch, lr=None):
        """One iteration of the loop Lightning would run: training_step + AdamW (+ the scheduler's multiplier)."""
        opt = self._opt if self._opt is not None else self.configure_optimizers()
        opt = opt[0][0] if isinstance(opt, tuple) else opt
        loss = self.training_step(batch)
        lr = float(self.learning_rate if lr is None else lr)
        if self.lr_schedule is not None:
            lr *= float(self.lr_schedule(self.trainer().P.step))
        opt.param_groups[0]["lr"] = lr
        opt.step()
        self.global_step += 1
        return loss

    def reset_noise_accs(self):
        dm = self.diffusion_model
        self.noisy_acc = {t: {"acc@1": [], "acc@5": []} for t in range(0, dm.num_timesteps, dm.log_every_t)}

    def on_validation_start(self):
        self.reset_noise_accs()

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0):
        loss, *_ = self.shared_step(batch, backward=False)
        for t in self.noisy_acc:
            _, logits, _, targets = self.shared_step(batch, t, backward=False)
            self.noisy_acc[t]["acc@1"].append(self.compute_top_k(logits, targets, k=1, reduction="mean"))
            self.noisy_acc[t]["acc@5"].append(self.compute_top_k(logits, targets, k=min(5, logits.shape[1]), reduction="mean"))
        return loss

    def configure_optimizers(self):
        """classifier.py:220-235: AdamW(learning_rate, weight_decay) over the classifier.  The step is ldmk_adamw over the flat packed
        buffer; a `scheduler_config` is instantiated and exposed as `lr_schedule` (step -> multiplier), as in ddpm.py here."""
        self._opt = _AdamWOfTrainer(self, float(self.learning_rate), float(self.weight_decay))
        if self.use_scheduler:
            self.lr_schedule = instantiate_from_config(self.scheduler_config).schedule
            return [self._opt], [dict(scheduler=self.lr_schedule, interval="step", frequency=1)]
        return self._opt

    def log_images(self, *args, **kwargs):
        raise NotImplementedError("NoisyLatentImageClassifier.log_images is not built")

    # ---- guidance -------------------------------------------------------------------------------------------
    def log_prob_grad(self, x_noisy, t, y):
        """The gradient of sum_b log p(y_b | x_b, t_b) w.r.t. x_noisy: one forward and one backward (want_dx) of the guidance
        trainer, with dlogits = onehot - softmax."""
        tr = self._guidance_trainer()
        logits = tr.forward(x_noisy.contiguous().float(), t.to(torch.int64), keep_tape=True)
        _, _, dl = T.cross_entropy(logits, y.to(logits.device, torch.int64).contiguous(), scale=-1.0)
        return tr.backward(dl)


class ClassifierGuidance:
    """`score_corrector=` for the DDIM, PLMS and DDPM entry points: Dhariwal & Nichol's epsilon form,
    e_t - sqrt(1 - abar_t) * scale * grad_x log p(y | x_t, t).  `y` comes from `corrector_kwargs` (or the constructor); the labels
    behind `c` are never guessed."""

    def __init__(self, classifier, scale=1.0, y=None):
        self.classifier, self.scale, self.y = classifier, float(scale), y

    def modify_score(self, model, e_t, x, t, c, y=None):
        y = self.y if y is None else y
        if y is None:
            raise ValueError("ClassifierGuidance: pass the labels as corrector_kwargs=dict(y=...) (or ClassifierGuidance(..., y=...))")
        y = torch.as_tensor(y, device=x.device)
        t = t.to(torch.int64)
        if y.dim() == 0:
            y = y.expand(x.shape[0])
        grad = self.classifier.log_prob_grad(x, t, y)
        sig = model.sqrt_one_minus_alphas_cumprod.to(x.device).gather(-1, t).reshape(-1, *([1] * (x.dim() - 1)))
        return e_t - sig * self.scale * grad
