"""Diagonal-Gaussian posterior of the KL first stage: drop-in for `ldm.modules.distributions.distributions`
(distributions.py:24-62 `DiagonalGaussianDistribution`, :65-92 `normal_kl`).

`parameters` are the encoder's moments (n, 2e, h, w): mean on channels [0, e), log-variance on [e, 2e).  On the GPU the
clamped log-variance, `std`, `var` and the sample all come from one elementwise kernel (`ldmk_gauss_posterior`); the three
tensors are produced together the first time one of them is read, a sample alone never materialises them.  `kl` and `nll`
are a few lines of torch over those tensors: the validation step of first-stage training reads `kl` from here, while the
training step takes the draw, the per-sample KL and their gradient from its own kernels (ldmk_gauss_kl_fwd / _bwd,
train_first_stage.py).  Moments on the CPU (fixtures, host-side checks of `kl` / `nll`) get the same attributes
from torch; sampling needs the GPU.
"""
import math

import torch

from . import lib as L
from . import ops


class DiagonalGaussianDistribution(object):
    def __init__(self, parameters, deterministic=False):
        if parameters.dim() != 4 or parameters.shape[1] % 2:
            raise ValueError(f"DiagonalGaussianDistribution: moments must be (n, 2e, h, w), got {tuple(parameters.shape)}")
        self.parameters = parameters
        self.deterministic = deterministic
        self.mean = parameters[:, :parameters.shape[1] // 2]
        self._lazy = None

    # ---- logvar / std / var: one launch for the three, on first use ------------------------------------------------
    def _moments(self):
        if self._lazy is None:
            p = self.parameters
            if p.is_cuda:
                with torch.no_grad():
                    o = ops.gauss_posterior(p.detach().float().contiguous(), logvar=True, std=True, var=True)
                lazy = (o["logvar"], o["std"], o["var"])
            else:
                logvar = p[:, p.shape[1] // 2:].clamp(-30.0, 20.0)
                lazy = (logvar, torch.exp(0.5 * logvar), torch.exp(logvar))
            if self.deterministic:
                zero = torch.zeros_like(self.mean)
                lazy = (lazy[0], zero, zero)
            self._lazy = lazy
        return self._lazy

    @property
    def logvar(self):
        return self._moments()[0]

    @property
    def std(self):
        return self._moments()[1]

    @property
    def var(self):
        return self._moments()[2]

    # ---- draws ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, noise=None, scale=1.0):
        """mean + std * noise, times `scale` (LatentDiffusion folds its scale_factor in here).  `noise`: the normal draw
        to use, default `torch.randn` on the moments' device."""
        p = self.parameters
        if not p.is_cuda:
            raise L.LdmkError("DiagonalGaussianDistribution.sample: CUDA tensors only (no CPU fallback)")
        if self.deterministic:
            noise = None                                   # std = 0: the draw is the mean
        elif noise is None:
            noise = torch.randn(self.mean.shape, device=p.device, dtype=torch.float32)
        else:
            noise = noise.to(p.device, torch.float32).contiguous()
        return ops.gauss_posterior(p.detach().float().contiguous(), noise=noise, scale=scale, z=True)["z"]

    def mode(self):
        return self.mean

    # ---- first-stage training losses (host-side torch) ---------------------------------------------------------------
    def kl(self, other=None):
        """KL(self || other) summed per sample; other=None: against the standard normal."""
        if self.deterministic:
            return torch.Tensor([0.])
        if other is None:
            terms = self.mean.pow(2) + self.var - 1.0 - self.logvar
        else:
            terms = ((self.mean - other.mean).pow(2) / other.var + self.var / other.var - 1.0 - self.logvar + other.logvar)
        return 0.5 * terms.sum(dim=[1, 2, 3])

    def nll(self, sample, dims=[1, 2, 3]):
        if self.deterministic:
            return torch.Tensor([0.])
        terms = math.log(2.0 * math.pi) + self.logvar + (sample - self.mean).pow(2) / self.var
        return 0.5 * terms.sum(dim=dims)


def normal_kl(mean1, logvar1, mean2, logvar2):
    """Elementwise KL(N(mean1, e^logvar1) || N(mean2, e^logvar2)); scalars broadcast against the tensor arguments."""
    like = next((a for a in (mean1, logvar1, mean2, logvar2) if isinstance(a, torch.Tensor)), None)
    assert like is not None, "at least one argument must be a Tensor"
    logvar1, logvar2 = (a if isinstance(a, torch.Tensor) else torch.tensor(a).to(like) for a in (logvar1, logvar2))
    return 0.5 * (-1.0 + logvar2 - logvar1 + torch.exp(logvar1 - logvar2) + (mean1 - mean2) ** 2 * torch.exp(-logvar2))
