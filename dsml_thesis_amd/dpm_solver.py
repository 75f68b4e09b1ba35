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

The rest of the reference's solver -- singlestep and singlestep_fixed, the noise-prediction form, solver type 'taylor', dynamic
thresholding, denoise_to_zero, a solve over [t_end, t_start] -- is on the object the reference has it on: `DPM_Solver`, made by
`DPMSolverSampler(model).solver(...)`, with `NoiseScheduleVP` as the reference's spelling of `DiscreteSchedule` (second half of
this file; one `method_table` row and one graph replay per model evaluation, `ldmk_dpm_stage`).
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

    def time_steps(self, skip_type, S, t_T=None, t_0=None):
        """get_time_steps (dpm_solver.py:405-431) from t_T (T = 1) down to t_0 (1/N), Python floats: S + 1 times."""
        t_T, t_0 = self.T if t_T is None else t_T, 1. / self.total_N if t_0 is None else t_0
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

    def solver(self, conditioning=None, unconditional_guidance_scale=1., unconditional_conditioning=None, predict_x0=False,
               thresholding=False, max_val=1., use_graph=False, policy_batch=None):
        """-> DPM_Solver over this sampler's model: what reference code builds by hand as NoiseScheduleVP + model_wrapper(...,
        'noise', 'classifier-free') + DPM_Solver(model_fn, ns, predict_x0, thresholding, max_val) (dpm_solver.py:352)."""
        return DPM_Solver(self, conditioning, unconditional_guidance_scale, unconditional_conditioning, predict_x0, thresholding,
                          max_val, use_graph, policy_batch)


# ------------------------------------------------------------------------------------------------------------------------------
# DPM_Solver: the reference's second public surface (dpm_solver.py:351-1124) -- singlestep ("DPM-Solver-fast"), singlestep_fixed and
# multistep, data- and noise-prediction form, solver types 'dpm_solver' and 'taylor', dynamic thresholding, denoise_to_zero and a
# solve over [t_end, t_start].  One table row per MODEL EVALUATION (`method_table`), one launch sequence per evaluation (UNet
# program, [predict x0, quantile,] ldmk_dpm_stage with its advance), a whole run = that many replays of one captured graph.
STAGE_ROW = 16      # floats per row (include/ldmk.h, ldmk_dpm_stage)
K_SS_FIRST, K_SS_MID, K_SS_LAST, K_SS_TAYLOR3, K_MS1, K_MS2, K_MS3, K_DENOISE = range(8)
F_X0, F_THRESHOLD = 1, 2
USES_KEEP, USES_RING = 1, 2
METHODS = ("multistep", "singlestep", "singlestep_fixed")
SOLVER_TYPES = ("dpm_solver", "taylor")
QUANTILE_P = 0.995  # dpm_solver.py:395, "a hyperparameter in the paper of Imagen"


def NoiseScheduleVP(schedule="discrete", betas=None, alphas_cumprod=None, **kwargs):
    """The reference's spelling (dpm_solver.py:6-109) of `DiscreteSchedule`; 'linear' and 'cosine' (continuous-time models) are not built."""
    if schedule != "discrete":
        raise NotImplementedError(f"NoiseScheduleVP: schedule {schedule!r} ('linear' / 'cosine', continuous-time models) is not built; "
                                  "the models here are trained on discrete timesteps ('discrete')")
    if betas is not None:                                  # dpm_solver.py:98-99
        return DiscreteSchedule(torch.exp(torch.cumsum(torch.log(1. - betas.detach().to("cpu", torch.float32)), dim=0)))
    assert alphas_cumprod is not None
    return DiscreteSchedule(alphas_cumprod)


def singlestep_orders(steps, order):
    """-> (the order of each outer step, K) of the singlestep solver with `steps` model evaluations
    (get_orders_and_timesteps_for_singlestep_solver, dpm_solver.py:471-490)."""
    if order == 3:
        K = steps // 3 + 1
        if steps % 3 == 0:
            return [3] * (K - 2) + [2, 1], K
        return [3] * (K - 1) + ([1] if steps % 3 == 1 else [2]), K
    if order == 2:
        if steps % 2 == 0:
            return [2] * (steps // 2), steps // 2
        return [2] * (steps // 2) + [1], steps // 2 + 1
    if order == 1:
        return [1] * steps, 1
    raise ValueError("'order' must be '1' or '2' or '3'.")


def method_table(alphas_cumprod, steps=20, order=3, skip_type="time_uniform", method="singlestep", lower_order_final=True,
                 predict_x0=False, solver_type="dpm_solver", thresholding=False, denoise_to_zero=False, t_start=None, t_end=None):
    """-> namespace(table [n_eval][STAGE_ROW] float32, kinds, orders, timesteps (the outer grid), r [(r1, r2) per outer step],
    t_eval / t_input [n_eval] (the continuous and the model time of every evaluation), uses).  Row j is the update that follows
    model evaluation j.  Every scalar is formed as the reference forms it -- one-element float32 tensors through the same torch
    operations in the same order (dpm_solver.py:386-399, 439-496, 504-857, 1071-1123); the reference's Python-float and 0-dim
    factors ((0.5 / r1), r2 / r1, (1. / r2)) and its sign go into the coefficient the way Python evaluates them there, left to right.
    Multistep order 3 with lower_order_final and fewer than 15 steps, which the reference cannot run (:773), runs 1, 2, 3, ..., 2, 1."""
    if method not in METHODS:
        raise NotImplementedError(f"DPM_Solver: method {method!r} is not built (multistep, singlestep, singlestep_fixed are)")
    if solver_type not in SOLVER_TYPES:
        raise ValueError("'solver_type' must be either 'dpm_solver' or 'taylor', got {}".format(solver_type))
    if skip_type not in SKIP_TYPES:
        raise ValueError(f"Unsupported skip_type {skip_type}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic'")
    if order not in (1, 2, 3):
        raise ValueError("Solver order must be 1 or 2 or 3, got {}".format(order))
    ns = DiscreteSchedule(alphas_cumprod)
    t_0 = 1. / ns.total_N if t_end is None else t_end
    t_T = ns.T if t_start is None else t_start
    x0 = bool(predict_x0)
    taylor = solver_type == "taylor"
    lead = (lambda t: torch.exp(ns.log_alpha(t))) if x0 else ns.std                    # alpha_t (x0 form) / sigma_t (eps form)
    c_x = (lambda s, t: ns.std(t) / ns.std(s)) if x0 else (lambda s, t: torch.exp(ns.log_alpha(t) - ns.log_alpha(s)))
    sg = (lambda v: -v) if x0 else (lambda v: v)                                       # exp / expm1 of -h (x0 form), of h (eps form)
    one = 1. if x0 else -1.                                                            # phi_2 = phi_1 / h + 1 (x0) / - 1 (eps)
    rows, t_eval, kinds, r_list = [], [], [], []

    def emit(t, kind, cx, c0, **cols):
        row = torch.zeros(STAGE_ROW, dtype=torch.float32)
        row[0], row[1], row[2], row[3], row[4] = torch.exp(ns.log_alpha(t)), ns.std(t), float(kind), cx, c0
        for col, v in cols.items():
            row[int(col[1:])] = v
        flags = (F_X0 if x0 else 0) | (F_THRESHOLD if (x0 and thresholding) else 0)
        if kind == K_DENOISE:                              # data_prediction_fn whatever the form (:498-502); it thresholds if asked
            flags = F_X0 | (F_THRESHOLD if thresholding else 0)
        row[14] = float(flags)
        rows.append(row)
        t_eval.append(t.reshape(1))
        kinds.append(kind)

    if method == "multistep":
        assert steps >= order                                        # dpm_solver.py:1078
        orders = order_schedule(steps, order, lower_order_final)
        ts = ns.time_steps(skip_type, steps, t_T, t_0)
        assert ts.shape[0] - 1 == steps
        tv = [ts[k].reshape(1) for k in range(steps + 1)]
        lam = [ns.lam(t) for t in tv]
        for k, o in enumerate(orders):
            s, t = tv[k], tv[k + 1]
            h = lam[k + 1] - lam[k]
            if o == 1:
                emit(s, K_MS1, c_x(s, t), lead(t) * torch.expm1(sg(h)))
                continue
            c0 = lead(t) * (torch.exp(sg(h)) - 1.)
            r0 = (lam[k] - lam[k - 1]) / h
            c1t = lead(t) * ((torch.exp(sg(h)) - 1.) / h + one)      # (x0: alpha_t ((exp(-h) - 1) / h + 1); eps: sigma_t ((exp(h) - 1) / h - 1))
            if o == 2:
                c1 = (c1t if x0 else -c1t) if taylor else -(0.5 * c0)
                emit(s, K_MS2, c_x(s, t), c0, c5=1. / r0, c9=c1)
            else:                                                    # (the third-order update ignores solver_type, :812-857)
                r1 = (lam[k - 1] - lam[k - 2]) / h
                c2 = lead(t) * ((torch.exp(sg(h)) - 1. + (h if x0 else -h)) / h ** 2 - 0.5)
                emit(s, K_MS3, c_x(s, t), c0, c5=1. / r0, c6=1. / r1, c7=r0 / (r0 + r1), c8=1. / (r0 + r1), c9=c1t if x0 else -c1t, c10=c2)
        outer = ts
    else:
        if method == "singlestep":
            orders, K = singlestep_orders(steps, order)
            if skip_type == "logSNR":                                # "to reproduce the results in DPM-Solver paper" (:491-493)
                outer = ns.time_steps(skip_type, K, t_T, t_0)
            else:
                outer = ns.time_steps(skip_type, steps, t_T, t_0)[torch.cumsum(torch.tensor([0] + orders), 0)]
        else:
            K = steps // order
            orders = [order] * K
            outer = ns.time_steps(skip_type, K, t_T, t_0)
        if outer.shape[0] - 1 < len(orders):               # order 1 under 'logSNR': K = 1 for `steps` updates (:486-493)
            raise ValueError(f"singlestep order {order} with skip_type 'logSNR' and steps={steps}: the reference's outer grid has "
                             f"{outer.shape[0] - 1} step(s) for {len(orders)} updates (dpm_solver.py:486-493; an IndexError there)")
        for i, o in enumerate(orders):
            s, t = outer[i].reshape(1), outer[i + 1].reshape(1)
            inner = ns.time_steps(skip_type, o, outer[i].item(), outer[i + 1].item())    # :1113-1120
            lam_in = ns.lam(inner)
            h_in = lam_in[-1] - lam_in[0]
            r1 = None if o <= 1 else (lam_in[1] - lam_in[0]) / h_in
            r2 = None if o <= 2 else (lam_in[2] - lam_in[0]) / h_in
            r_list.append((0. if r1 is None else r1.item(), 0. if r2 is None else r2.item()))
            lam_s, lam_t = ns.lam(s), ns.lam(t)
            h = lam_t - lam_s
            phi_1 = torch.expm1(sg(h))
            if o == 1:
                emit(s, K_SS_FIRST, c_x(s, t), lead(t) * phi_1)
                continue
            s1 = ns.inverse_lam(lam_s + r1 * h)
            phi_11 = torch.expm1(sg(r1) * h)
            emit(s, K_SS_FIRST, c_x(s, s1), lead(s1) * phi_11)
            if o == 2:
                c0 = lead(t) * phi_1
                if taylor:
                    k = (1. / r1) * (lead(t) * ((torch.exp(sg(h)) - 1.) / h + one))
                    k = k if x0 else -k
                else:
                    k = -((0.5 / r1) * c0)
                emit(s1, K_SS_LAST, c_x(s, t), c0, c5=k)
                continue
            s2 = ns.inverse_lam(lam_s + r2 * h)
            phi_12 = torch.expm1(sg(r2) * h)
            phi_22 = torch.expm1(sg(r2) * h) / (r2 * h) + one
            phi_2 = phi_1 / h + one
            phi_3 = phi_2 / h - 0.5
            k = r2 / r1 * (lead(s2) * phi_22)
            emit(s1, K_SS_MID, c_x(s, s2), lead(s2) * phi_12, c5=k if x0 else -k)
            c1 = lead(t) * phi_2
            if taylor:
                emit(s2, K_SS_TAYLOR3, c_x(s, t), lead(t) * phi_1, c5=1. / r1, c6=1. / r2, c7=r1, c8=r2, c9=c1 if x0 else -c1,
                     c10=lead(t) * phi_3, c11=r2 - r1)
            else:
                k = (1. / r2) * c1
                emit(s2, K_SS_LAST, c_x(s, t), lead(t) * phi_1, c5=k if x0 else -k)
    t_last = outer[-1].reshape(1)
    if denoise_to_zero:                                    # one more evaluation at t_0 (:1122-1123)
        t_last = torch.ones((1,)) * t_0
        emit(t_last, K_DENOISE, 0., 0.)
    table = torch.stack(rows)
    t_input = torch.cat([ns.model_time(t) for t in t_eval])
    table[:-1, 15] = t_input[1:]
    table[-1, 15] = ns.model_time(t_last)[0]
    uses = (USES_KEEP if any(k <= K_SS_TAYLOR3 for k in kinds) else 0) | (USES_RING if any(K_MS1 <= k <= K_MS3 for k in kinds) else 0)
    return types.SimpleNamespace(table=table, kinds=kinds, orders=orders, timesteps=outer, r=r_list, t_eval=torch.cat(t_eval),
                                 t_input=t_input, uses=uses)


class DPM_Solver:
    """Drop-in for the reference's DPM_Solver (dpm_solver.py:351-1124), bound to a model instead of a Python `model_fn`: the model
    evaluation is the float-time launch program, with classifier-free guidance by batch doubling, so there is nothing to wrap.
    Made by `DPMSolverSampler(model).solver(...)`."""

    def __init__(self, sampler, conditioning=None, unconditional_guidance_scale=1., unconditional_conditioning=None, predict_x0=False,
                 thresholding=False, max_val=1., use_graph=False, policy_batch=None):
        self.sampler, self.model = sampler, sampler.model
        self.noise_schedule = DiscreteSchedule(sampler.alphas_cumprod)
        self.conditioning, self.scale, self.unconditional_conditioning = conditioning, unconditional_guidance_scale, unconditional_conditioning
        self.predict_x0, self.thresholding, self.max_val = bool(predict_x0), bool(thresholding), float(max_val)
        self.use_graph, self.policy_batch = bool(use_graph), policy_batch
        self._tables = self.model.__dict__.setdefault("_dpm_method_tables", {})       # shared like DPMSolverSampler._dpm_tables

    def _table_for(self, **kw):
        dev = self.model.device
        key = tuple(sorted(kw.items())) + (str(dev),)
        if key not in self._tables:
            tab = method_table(self.sampler.alphas_cumprod, **kw)
            tab.key, tab.device_table = key, tab.table.to(dev)
            self._tables[key] = tab
        return self._tables[key]

    @torch.no_grad()
    def sample(self, x, steps=20, t_start=None, t_end=None, order=3, skip_type="time_uniform", method="singlestep",
               lower_order_final=True, denoise_to_zero=False, solver_type="dpm_solver", atol=0.0078, rtol=0.05, intermediates=False):
        """dpm_solver.py:965-1124 -> the latent at t_end.  intermediates=True: (latent, {"x_inter": the latent entering every model
        evaluation plus the final one, "t_input": the model time of every evaluation[, "s": the thresholding scale of every
        evaluation and sample]}).  `atol` / `rtol` belong to 'adaptive'."""
        if method == "adaptive":
            raise NotImplementedError("DPM_Solver: method 'adaptive' (DPM-Solver-12 / -23) is not built: its step size depends on a "
                                      "device norm every step, so it is a host-synchronised loop with the schedule inverted on the device")
        if method not in METHODS:
            raise ValueError(f"Got wrong method {method}")
        if (method == "multistep" and self.predict_x0 and solver_type == "dpm_solver" and not self.thresholding and not denoise_to_zero
                and t_start is None and t_end is None and skip_type in SKIP_TYPES and order in (1, 2, 3)):
            # the branch DPMSolverSampler.sample runs: its own loop and kernel (ldmk_dpm_step), so the two agree bit for bit
            # (the compiler contracts that kernel's products and sums where csrc/dpm.hip is built without contraction)
            assert steps >= order                                    # dpm_solver.py:1078
            out, inter = self.sampler._dpm_loop(self.conditioning, tuple(x.shape), x, int(steps), int(order), skip_type,
                                                bool(lower_order_final), self.scale, self.unconditional_conditioning, self.use_graph,
                                                self.policy_batch, bool(intermediates))
            if not intermediates:
                return out
            tab = self.sampler._table_for(int(steps), int(order), skip_type, bool(lower_order_final))
            return out, {"x_inter": inter, "t_input": tab.t_input[:int(steps)].to(out.device)}
        tab = self._table_for(steps=int(steps), order=order, skip_type=skip_type, method=method, lower_order_final=bool(lower_order_final),
                              predict_x0=self.predict_x0, solver_type=solver_type, thresholding=self.thresholding,
                              denoise_to_zero=bool(denoise_to_zero), t_start=None if t_start is None else float(t_start),
                              t_end=None if t_end is None else float(t_end))
        out, inter = self._loop(x, tab, bool(intermediates))
        return (out, inter) if intermediates else out

    @rerun_if_flags_tripped(lambda self: self.model.model.diffusion_model)
    def _loop(self, x, tab, want_inter):
        r = self.sampler._prepare_run(self.conditioning, tuple(x.shape), x, self.scale, self.unconditional_conditioning,
                                      self.policy_batch, "dpm_methods", float_time=True)
        dev, b, img0, cfg, pg, img, eps, run_net = r.dev, r.b, r.img0, r.cfg, r.pg, r.img, r.eps, r.run_net
        table, n_eval, uses = tab.device_table, tab.table.shape[0], tab.uses
        t_first = float(tab.t_input[0])
        thresholded = bool((tab.table[:, 14].to(torch.int32) & F_THRESHOLD).any())
        lib = pg.lib
        t_buf = pg.inputs["t_f32"]
        n_ts = t_buf.numel()
        scale, max_val = float(self.scale), self.max_val
        per = img0[0].numel()
        # keep = [x_s | m_s | m_s1] of the current singlestep outer step; ring[k % 3] = the model value of multistep row k
        st = r.state((cfg, scale, tab.key, max_val if thresholded else None, self.use_graph), lambda: dict(
            model_out=torch.empty_like(img0), step_idx=torch.zeros(1, dtype=torch.int32, device=dev),
            keep=torch.empty((3,) + tuple(img0.shape), device=dev) if uses & USES_KEEP else None,
            ring=torch.empty((3,) + tuple(img0.shape), device=dev) if uses & USES_RING else None,
            x0_pre=torch.empty_like(img0) if thresholded else None, s=torch.empty(b, device=dev) if thresholded else None))
        model_out, step_idx, keep, ring, x0_pre, s = (st[k] for k in ("model_out", "step_idx", "keep", "ring", "x0_pre", "s"))
        ptr = lambda t: 0 if t is None else t.data_ptr()

        def reset_state():
            r.seed()
            step_idx.zero_()                               # row 0 is a stage 0 / an order-1 row: keep and ring are dead from here
            t_buf.fill_(t_first)

        def one_eval():
            run_net()
            stream = torch.cuda.current_stream().cuda_stream
            if thresholded:
                L.check(lib.ldmk_dpm_predict_x0(img.data_ptr(), eps.data_ptr(), table.data_ptr(), step_idx.data_ptr(), scale,
                                                1 if cfg else 0, x0_pre.data_ptr(), per, b, n_eval, stream), "ldmk_dpm_predict_x0")
                L.check(lib.ldmk_abs_quantile_rows(x0_pre.data_ptr(), b, per, QUANTILE_P, max_val, s.data_ptr(), stream),
                        "ldmk_abs_quantile_rows")
            rc = lib.ldmk_dpm_stage(img.data_ptr(), eps.data_ptr(), table.data_ptr(), step_idx.data_ptr(), scale, 1 if cfg else 0,
                                    ptr(x0_pre), ptr(s), ptr(keep), ptr(ring), img.data_ptr(), model_out.data_ptr(), per, b,
                                    t_buf.data_ptr(), n_ts, 1, n_eval, uses, stream)
            L.check(rc, "ldmk_dpm_stage")
            r.share_latent()                               # (dpm_solver.py:340)

        reset_state()
        step = r.stepper(st, one_eval, reset_state, self.use_graph)
        inter = {"x_inter": [img0.clone()], "t_input": []} if want_inter else None
        if want_inter and thresholded:
            inter["s"] = []                                # (thresholded runs: s per evaluation and sample)
        for _ in range(n_eval):
            if want_inter:
                inter["t_input"].append(t_buf[:1].clone())
            step()
            if want_inter:
                inter["x_inter"].append(img.clone())
                if thresholded:
                    inter["s"].append(s.clone())
        if want_inter:
            inter["t_input"] = torch.cat(inter["t_input"])
        return img.clone(), inter
