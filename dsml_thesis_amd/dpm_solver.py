"""DPMSolverSampler: drop-in for the reference's DPM-Solver sampler
  talking_face/ldm/models/diffusion/dpm_solver/sampler.py:8-81      (the sampler: one hard-wired DPM_Solver.sample call)
  talking_face/ldm/models/diffusion/dpm_solver/dpm_solver.py        (NoiseScheduleVP 'discrete', model_wrapper, DPM_Solver)

What is built is the branch the reference's sampler takes: the multistep DPM-Solver++ (data prediction, solver type
'dpm_solver', no thresholding) on the discrete schedule, orders 1-3, with classifier-free guidance by batch doubling.  The solver
works in continuous time t in [1/N, 1] and evaluates the UNet at the REAL-valued model time (t - 1/N) 1000, so the loop runs over
the float-time launch program (`UNetModel.program(..., float_time=True)`).  It evaluates the model once per step, the first step
included, so every step is the same sequence -- UNet program, `ldmk_dpm_step`, advance -- and a whole run is S replays of one
captured graph.  Everything before the first step is `sampling_loop.prepare_run` (through `DDIMSampler._prepare_run`), so every
conditioning_key and `split_input_params` work as under DDIM; loop state and graph capture are that module's `Run`.

The scalars of a run -- time steps, lambda, alpha, sigma, the per-step coefficients -- are one host table (`step_table`), computed in
torch float32 on the CPU with the reference's operations in the reference's order: h is a difference of two lambda of magnitude ~5,
so a table rounded from float64 would differ from the reference's scalars by 1e-6 .. 1e-5 relative and that compounds.

Additions over the reference, as keywords of `sample`: `order=`, `skip_type=`, `lower_order_final=`, `use_graph=`, `policy_batch=`,
`intermediates=`.
"""
import types

import torch

from . import lib as L
from .ddim import DDIMSampler
from .unet import rerun_if_flags_tripped

ROW = 12            # floats per table row (include/ldmk.h, ldmk_dpm_step)
SKIP_TYPES = ("time_uniform", "logSNR", "time_quadratic")


class DiscreteSchedule:
    """NoiseScheduleVP('discrete', alphas_cumprod=...) (dpm_solver.py:97-109, 125-170): log alpha_t is the piecewise-linear
    interpolation of 0.5 log(alphas_cumprod) over linspace(0, 1, N + 1)[1:].  CPU, float32; times are 1-D tensors."""

    def __init__(self, alphas_cumprod):
        ac = alphas_cumprod.detach().to("cpu", torch.float32)
        self.log_alphas = 0.5 * torch.log(ac)
        self.total_N = self.log_alphas.shape[0]
        self.T = 1.
        self.t_array = torch.linspace(0., 1., self.total_N + 1)[1:]

    @staticmethod
    def interpolate(x, xp, yp):
        """Piecewise-linear y(x) through the keypoints (xp, yp), xp ascending; beyond either end the outermost segment is
        continued (interpolate_fn, dpm_solver.py:1132-1171).  The segment is found the way the reference finds it -- x is put in
        front of the keypoints, the lot is sorted, and x's place in the order names the segment -- so that an x that EQUALS a
        keypoint (t = 1, t = 1/N) lands on the same side of it and the result has the same bits."""
        M, K = x.shape[0], xp.shape[0]
        both = torch.cat([x.reshape(M, 1, 1), xp.reshape(1, 1, K).repeat(M, 1, 1)], dim=2)
        _, perm = torch.sort(both, dim=2)
        pos = torch.argmin(perm, dim=2).reshape(M)                   # where x (entry 0) landed: 0 .. K
        j0 = torch.where(pos == 0, torch.zeros_like(pos), torch.where(pos == K, torch.full_like(pos, K - 2), pos - 1))
        x0, x1, y0, y1 = xp[j0], xp[j0 + 1], yp[j0], yp[j0 + 1]
        return y0 + (x - x0) * (y1 - y0) / (x1 - x0)

    def log_alpha(self, t):
        return self.interpolate(t.reshape(-1), self.t_array, self.log_alphas)

    def alpha(self, t):
        return torch.exp(self.log_alpha(t))

    def std(self, t):
        return torch.sqrt(1. - torch.exp(2. * self.log_alpha(t)))

    def lam(self, t):
        la = self.log_alpha(t)
        return la - 0.5 * torch.log(1. - torch.exp(2. * la))

    def inverse_lam(self, lam):
        la = -0.5 * torch.logaddexp(torch.zeros((1,)), -2. * lam)
        return self.interpolate(la.reshape(-1), torch.flip(self.log_alphas, [0]), torch.flip(self.t_array, [0]))

    def model_time(self, t):
        """dpm_solver.py:278-287: continuous t in [1/N, 1] -> the UNet's timestep in [0, 1000 (N - 1) / N]."""
        return (t - 1. / self.total_N) * 1000.

    def time_steps(self, skip_type, S):
        """get_time_steps (dpm_solver.py:405-431) from T = 1 down to 1/N: S + 1 times."""
        t_T, t_0 = self.T, 1. / self.total_N
        if skip_type == "logSNR":
            lam_T, lam_0 = self.lam(torch.tensor(t_T)), self.lam(torch.tensor(t_0))
            return self.inverse_lam(torch.linspace(lam_T.item(), lam_0.item(), S + 1))
        if skip_type == "time_uniform":
            return torch.linspace(t_T, t_0, S + 1)
        if skip_type == "time_quadratic":
            return torch.linspace(t_T ** (1. / 2), t_0 ** (1. / 2), S + 1).pow(2)
        raise ValueError(f"Unsupported skip_type {skip_type}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic'")


def order_schedule(steps, order, lower_order_final=True):
    """The order of each of the `steps` multistep updates (dpm_solver.py:1078-1105): the first order - 1 steps ramp up from 1;
    step number `step` (from 1) after that has order min(order, steps + 1 - step) when lower_order_final and steps < 15."""
    assert order in (1, 2, 3), f"order {order}: the multistep solver has orders 1, 2 and 3"
    assert steps >= order                                            # dpm_solver.py:1078
    orders = list(range(1, order))
    for step in range(order, steps + 1):
        orders.append(min(order, steps + 1 - step) if (lower_order_final and steps < 15) else order)
    return orders


def step_table(alphas_cumprod, steps, order=2, skip_type="time_uniform", lower_order_final=True):
    """-> namespace(table [steps][ROW] float32, orders, timesteps [steps + 1], t_input [steps + 1], lam / alpha / sigma
    [steps + 1]).  Row k is the step from s = t_k to t = t_{k+1}; every scalar is formed as the reference forms it -- one-element
    float32 tensors through the same torch operations in the same order (dpm_solver.py:386-399, 517-533, 771-790, 821-849)."""
    ns = DiscreteSchedule(alphas_cumprod)
    orders = order_schedule(steps, order, lower_order_final)
    ts = ns.time_steps(skip_type, steps)
    assert ts.shape[0] - 1 == steps
    tv = [ts[k].reshape(1) for k in range(steps + 1)]
    lam = [ns.lam(t) for t in tv]
    sigma = [ns.std(t) for t in tv]
    alpha = [torch.exp(ns.log_alpha(t)) for t in tv]
    t_input = [ns.model_time(t) for t in tv]
    table = torch.zeros(steps, ROW, dtype=torch.float32)
    for k in range(steps):
        o = orders[k]
        h = lam[k + 1] - lam[k]
        row = table[k]
        row[0], row[1], row[2] = alpha[k], sigma[k], float(o)
        row[3] = sigma[k + 1] / sigma[k]
        row[4] = alpha[k + 1] * (torch.expm1(-h) if o == 1 else (torch.exp(-h) - 1.))
        if o >= 2:
            r0 = (lam[k] - lam[k - 1]) / h
            row[5] = 1. / r0
        if o == 3:
            r1 = (lam[k - 1] - lam[k - 2]) / h
            row[6], row[7], row[8] = 1. / r1, r0 / (r0 + r1), 1. / (r0 + r1)
            row[9] = alpha[k + 1] * ((torch.exp(-h) - 1.) / h + 1.)
            row[10] = alpha[k + 1] * ((torch.exp(-h) - 1. + h) / h ** 2 - 0.5)
        row[11] = t_input[k + 1]
    cat = lambda xs: torch.cat(xs)
    return types.SimpleNamespace(table=table, orders=orders, timesteps=ts, t_input=cat(t_input), lam=cat(lam), alpha=cat(alpha),
                                 sigma=cat(sigma))


class DPMSolverSampler(DDIMSampler):
    def __init__(self, model, **kwargs):
        super().__init__(model, **kwargs)
        self.register_buffer("alphas_cumprod", model.alphas_cumprod.clone().detach().to(torch.float32))
        # host + device tables, shared by every sampler of this model: captured graphs keep pointing at the device copy
        self._dpm_tables = model.__dict__.setdefault("_dpm_tables", {})

    def _table_for(self, steps, order, skip_type, lower_order_final):
        dev = self.model.device
        key = (int(steps), int(order), skip_type, bool(lower_order_final), str(dev))
        if key not in self._dpm_tables:
            tab = step_table(self.alphas_cumprod, steps, order, skip_type, lower_order_final)
            tab.key, tab.device_table = key, tab.table.to(dev)
            self._dpm_tables[key] = tab
        return self._dpm_tables[key]

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, order=2, skip_type="time_uniform", lower_order_final=True, method="multistep",
               predict_x0=True, thresholding=False, solver_type="dpm_solver", use_graph=False, policy_batch=None,
               intermediates=False, **kwargs):
        """sampler.py:22-81 -> (x, None).  Like the reference, `mask`, `x0`, `quantize_x0`, `eta`, `temperature`, `noise_dropout`,
        `score_corrector`, `callback` and `img_callback` (and normals_sequence, corrector_kwargs, verbose, log_every_t) are
        accepted and IGNORED: the reference's sampler never passes them on (:55-82).  The defaults are its hard-wired call
        (multistep, order 2, time_uniform, lower_order_final, data prediction, 'dpm_solver').
        intermediates=True: the second value is {"x_inter": [...]}, the latent entering every model evaluation plus the final one."""
        if method != "multistep":
            raise NotImplementedError(f"DPMSolverSampler: method {method!r} (singlestep / singlestep_fixed / adaptive) is not built; "
                                      "the reference's sampler runs 'multistep' only")
        if not predict_x0:
            raise NotImplementedError("DPMSolverSampler: predict_x0=False (the noise-prediction form, DPM-Solver) is not built; the "
                                      "reference's sampler runs the data-prediction form, DPM-Solver++")
        if thresholding:
            raise NotImplementedError("DPMSolverSampler: thresholding (dynamic thresholding of x0) is not built")
        if solver_type != "dpm_solver":
            raise NotImplementedError(f"DPMSolverSampler: solver_type {solver_type!r} ('taylor') is not built")
        if skip_type not in SKIP_TYPES:
            raise ValueError(f"Unsupported skip_type {skip_type}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic'")
        if order not in (1, 2, 3):
            raise ValueError(f"Solver order must be 1 or 2 or 3, got {order}")
        assert S >= order                                            # dpm_solver.py:1078
        if conditioning is not None:
            first = conditioning[list(conditioning.keys())[0]] if isinstance(conditioning, dict) else conditioning
            first = first[0] if isinstance(first, (list, tuple)) else first
            if first.shape[0] != batch_size:
                print(f"Warning: Got {first.shape[0]} conditionings but batch-size is {batch_size}")
        C_, H, W_ = shape
        out, inter = self._dpm_loop(conditioning, (batch_size, C_, H, W_), x_T, int(S), int(order), skip_type, bool(lower_order_final),
                                    unconditional_guidance_scale, unconditional_conditioning, use_graph, policy_batch,
                                    bool(intermediates))
        return out, ({"x_inter": inter} if intermediates else None)

    @rerun_if_flags_tripped(lambda self: self.model.model.diffusion_model)
    def _dpm_loop(self, cond, shape, x_T, S, order, skip_type, lower_order_final, unconditional_guidance_scale,
                  unconditional_conditioning, use_graph, policy_batch, want_inter):
        r = self._prepare_run(cond, shape, x_T, unconditional_guidance_scale, unconditional_conditioning, policy_batch, "dpm",
                              float_time=True)
        dev, b, img0, cfg, pg, img, eps, run_net = r.dev, r.b, r.img0, r.cfg, r.pg, r.img, r.eps, r.run_net
        tab = self._table_for(S, order, skip_type, lower_order_final)
        table, t_first, max_order = tab.device_table, float(tab.t_input[0]), max(tab.orders)
        lib = pg.lib
        t_buf = pg.inputs["t_f32"]
        n_ts = t_buf.numel()                               # (patch-wise: L*nb entries, all the current model time)
        scale = float(unconditional_guidance_scale)
        # ring[k % 3] = the data prediction of step k (ldmk_dpm_step); step_idx = the current step
        st = r.state((cfg, scale, tab.key, bool(use_graph)), lambda: dict(
            pred_x0=torch.empty_like(img0), ring=torch.empty((3,) + tuple(img0.shape), device=dev),
            step_idx=torch.zeros(1, dtype=torch.int32, device=dev)))
        pred_x0, ring, step_idx = st["pred_x0"], st["ring"], st["step_idx"]
        per = img0[0].numel()

        def reset_state():
            r.seed()
            step_idx.zero_()                               # row 0 is of order 1: the ring's contents are dead from here
            t_buf.fill_(t_first)

        def one_step():
            run_net()
            rc = lib.ldmk_dpm_step(img.data_ptr(), eps.data_ptr(), table.data_ptr(), step_idx.data_ptr(), scale, 1 if cfg else 0,
                                   ring.data_ptr(), img.data_ptr(), pred_x0.data_ptr(), per, b, t_buf.data_ptr(), n_ts, 1, S,
                                   max_order, torch.cuda.current_stream().cuda_stream)
            L.check(rc, "ldmk_dpm_step")
            r.share_latent()                               # (dpm_solver.py:340)

        reset_state()
        step = r.stepper(st, one_step, reset_state, use_graph)
        x_inter = [img0.clone()] if want_inter else None
        for _ in range(S):
            step()
            if want_inter:
                x_inter.append(img.clone())
        return img.clone(), x_inter
