"""What the device-resident sampling loops have in common -- `DDIMSampler.ddim_sampling`, `PLMSSampler._plms_loop`,
`DPMSolverSampler._dpm_loop` and `LatentDiffusion.p_sample_loop` -- and no sampler's maths.

  prepare_run   everything before the first step -> a `Run`
  Run           the latent in the UNet's input buffer and its second guidance half, loop state on the launch program, and the
                step callable (the step function, or the replay of its captured hipGraph)
  MaskBlend, score_source, quantize_fixup, log_step, check_conditioning
                the reference's rarely used options and the `sample()` preamble, as the DDIM and PLMS loops share them

A sampler keeps its step functions with their `ldmk_*_step` launch, the reset of its counters, its state's buffers and key, and
its host loop (which noise is fed when, the order of callbacks and intermediates).  Nothing here is told which sampler calls it.
"""
import types

import torch

from . import lib as L
from .engine import GraphedProgram

C12, C34 = "class_label_&_audio", "motion_&_id"


def is_adm(model):
    return getattr(model.model, "conditioning_key", None) == "adm"


def require_eps_model(model, who):
    """The DDIM, PLMS and DPM-Solver updates and the two fine-tunes take the network output as the noise estimate, as the reference's
    do whatever the model's parameterization (ddim.py:165-191 reads e_t = apply_model(...)).  Over an x0-prediction model that
    is a wrong sample, not an error, in the reference; here it is an error.  The ancestral loop (p_sample_loop) handles x0."""
    p = getattr(model, "parameterization", "eps")
    if p != "eps":
        raise NotImplementedError(f"{who}: the model predicts {p!r}, and this update reads the network output as eps "
                                  "(sample an x0-prediction model with LatentDiffusion.p_sample_loop / sample)")


def labels(cond):
    """conditioning_key 'adm': the class-label vector y (B,) out of whatever form apply_model accepts (ddpm.py:893-994 wraps a
    tensor as c_crossattn = [y]; DiffusionWrapper takes c_crossattn[0], :1417-1419)."""
    if isinstance(cond, dict):
        cond = cond.get("c_crossattn")
    if isinstance(cond, (list, tuple)):
        cond = cond[0]
    return cond


def split_cond(model, cond):
    """-> (crossattn context (B,L,D), c_concat (B,C,H,W) or None); 'adm': (class labels (B,), None)."""
    if is_adm(model):
        return labels(cond), None
    if isinstance(cond, dict):
        if C12 in cond:                      # TF sampler conditioning, ddim2cond.py:165
            return cond[C12], cond[C34]
        cc = cond.get("c_crossattn")
        ct = cond.get("c_concat")
        cc = torch.cat(cc, 1) if isinstance(cc, (list, tuple)) else cc
        ct = torch.cat(ct, 1) if isinstance(ct, (list, tuple)) else ct
        return cc, ct
    if isinstance(cond, (list, tuple)):
        cond = torch.cat(list(cond), 1)
    if cond is not None and getattr(model.model, "conditioning_key", None) == "concat":
        return None, cond                    # DiffusionWrapper 'concat': the conditioning is the channel concat (ddpm.py:1407-1409)
    return cond, None


def prepare_run(model, cond, shape, x_T, unconditional_guidance_scale, unconditional_conditioning, policy_batch, loops_name,
                float_time=False):
    """What every sampling loop does before its first step: start noise, conditioning split, guidance doubling, 'adm' labels, the
    launch program (or the patch-wise evaluator) with its conditioning written and its context program run, and the per-program
    dict `loops` that holds loop state under `loops_name` (one name per kind of loop, so the loops never meet each other's
    state) -> Run.  `float_time`: the program whose timestep input is the fp32 `t_f32`.  `policy_batch`: the batch size tile plans
    are made for (None: the run's own), or "keep": `unet.policy_batch` stays what it is."""
    dev = model.device
    unet = model.model.diffusion_model
    b = shape[0]
    img0 = torch.randn(shape, device=dev) if x_T is None else x_T.to(dev, torch.float32)
    ctx, cat = split_cond(model, cond)
    cfg = not (unconditional_conditioning is None or unconditional_guidance_scale == 1.)
    nb = 2 * b if cfg else b
    y_in = None
    if is_adm(model):
        # class-conditional model (ddpm.py:1417-1419): the conditioning is the label vector y, which reaches the UNet as rows of
        # its label embedding added to the timestep embedding -- constant over the run, written once into the program's
        # `y_emb` input; guidance doubles it as [uncond | cond] like any conditioning (ddim.py:175)
        y_in = ctx if not cfg else torch.cat([split_cond(model, unconditional_conditioning)[0], ctx])
        assert y_in is not None and y_in.dim() == 1 and cat is None, "conditioning_key 'adm': conditioning = class labels (B,)"
        ctx_in, cat_in = None, None
    elif cfg:
        uc, ucat = split_cond(model, unconditional_conditioning)
        if ctx is None:                                # 'concat' conditioning: the guidance halves differ in the concat tensor
            ctx_in, cat_in = None, torch.cat([ucat, cat])
        else:
            ctx_in = torch.cat([uc, ctx])              # ddim.py:175: [uncond | cond]
            cat_in = None if cat is None else torch.cat([cat] * 2)
    else:
        ctx_in, cat_in = ctx, cat
    ncat = 0 if cat_in is None else cat_in.shape[1]
    L_ctx = 0 if ctx_in is None else ctx_in.shape[1]          # 0: unconditional UNet (no cross-attention)
    policy_nb = policy_batch if policy_batch in (None, "keep") else (2 * policy_batch if cfg else policy_batch)
    y_emb = None if y_in is None else unet.label_emb.weight.detach().float()[y_in.to(dev, torch.int64)]
    if hasattr(model, "split_input_params"):
        # patch-wise (ddpm.py:904-986): the latent lives in a full-size buffer of nb items ([uncond | cond] under guidance, so
        # the update kernels' contract holds); one step = unfold -> the program at batch L*nb -> fold -> the update on the
        # full-size tensors.  Context / concat crops are written once per run.
        pe = model._patched_eval(nb, shape[1], shape[2], shape[3], L_ctx, ncat, policy_batch=policy_nb, float_time=float_time)
        pg = pe.pg
        pe.set_cond(ctx_in, cat_in, y_emb)
        x_buf, eps, run_net = pe.x, pe.eps, pe.run
        loops = pe.loops.setdefault(loops_name, {})    # (never the plain loop's state of the same program)
    else:
        if policy_nb != "keep":
            unet.policy_batch = policy_nb
        pg = unet.program(nb, shape[2], shape[3], L_ctx, ncat, float_time=float_time)
        x_buf, eps, run_net = pg.inputs["x"], pg.outputs["eps"], pg.run
        if L_ctx:
            pg.inputs["context"].copy_(ctx_in.reshape(nb * L_ctx, -1))
        if ncat:
            pg.inputs["c_concat"].copy_(cat_in)
        if y_emb is not None:
            pg.inputs["y_emb"].copy_(y_emb)
        pg.ctx_program.run()                           # context-only projections: once per sample() call
        # loop state (buffers, the captured step) lives ON the launch program it was captured over and dies with it: when the
        # model drops its programs (a re-pack, an arithmetic fall-back) nothing keeps the old workspace or its hipGraph alive,
        # and a new program can never be handed buffers of another batch size (rounds 2-4 keyed a sampler-side cache by id(pg))
        loops = pg.__dict__.setdefault(f"_{loops_name}_loops", {})
    return Run(dev=dev, b=b, img0=img0, cfg=cfg, pg=pg, x_buf=x_buf, eps=eps, run_net=run_net, loops=loops, img=x_buf[:b])


class Run(types.SimpleNamespace):
    """One prepared run.  `img` = `x_buf[:b]`: the latent lives in the UNet's input buffer (patch-wise: the full-size one); under
    guidance `x_buf[b:]` is its second half, which sees the same latent (ddim.py:173)."""

    def seed(self):                                    # the start noise, into both guidance halves
        self.img.copy_(self.img0)
        if self.cfg:
            self.x_buf[self.b:].copy_(self.img0)

    def share_latent(self):                            # after an update of `img`
        if self.cfg:
            self.x_buf[self.b:].copy_(self.img)

    def state(self, key, make, cached=True):
        """The loop-state dict under `key`: `make()` plus a "graph" entry, at first use.  cached=False: a fresh one that is not
        stored (option runs capture their own tensors: never cached)."""
        st = self.loops.get(key) if cached else None
        if st is None:
            st = dict(make(), graph=None)
            if cached:
                self.loops[key] = st
        return st

    def stepper(self, st, step, reset, use_graph, draw_first=None):
        """What the host loop calls once per step: `step`, or (use_graph) the replay of its hipGraph, captured at first use and
        followed by `reset()` because warm-up and capture advanced the device state.  `draw_first`: the noise draws that an eager
        loop makes before `step()`; they go inside the captured step."""
        if not use_graph:
            return step
        if st["graph"] is None:
            def step_with_noise():
                draw_first()
                step()
            st["graph"] = GraphedProgram(step if draw_first is None else step_with_noise)
            reset()
        return st["graph"].replay


class MaskBlend:
    """mask / x0: the inpainting blend before every step, `img = q_sample(x0, t) * mask + (1 - mask) * img` (ddim.py:143-146,
    plms.py:147-150), the timestep read from the device-side vector.  `mnz` is q_sample's noise: `mask_noise[i]` where that
    per-step list is given (parity with a seeded reference run), else a draw per step."""

    def __init__(self, run, model, mask, x0, mask_noise):
        assert x0 is not None, "mask needs x0 (ddim.py:144, plms.py:148)"
        self.run, self.noise = run, mask_noise
        self.mask = mask.to(run.dev, torch.float32).expand(run.img0.shape).contiguous()
        self.x0 = x0.to(run.dev, torch.float32)
        self.mnz = torch.zeros_like(run.img0)          # (zeros: the graph warm-up steps run before the first fill)
        self.sqrt_ac, self.sqrt_1mac = model.sqrt_alphas_cumprod, model.sqrt_one_minus_alphas_cumprod

    def blend(self, t_buf):
        r, b = self.run, self.run.b
        tcur = t_buf[:b]
        img_orig = self.sqrt_ac.gather(-1, tcur).view(b, 1, 1, 1) * self.x0 + self.sqrt_1mac.gather(-1, tcur).view(b, 1, 1, 1) * self.mnz
        r.img.copy_(img_orig * self.mask + (1. - self.mask) * r.img)
        r.share_latent()

    def feed(self, i):                                 # before step i: the given noise, if there is a list
        if self.noise is not None:
            self.mnz.copy_(self.noise[i])

    def draw(self):                                    # before a step, or first thing inside a captured one: else a draw
        if self.noise is None:
            self.mnz.normal_()


def score_source(run, model, score_corrector, corrector_kwargs, cond, scale, t_buf):
    """-> callable for after `run_net()`: (pointer to the score for the update kernel, its cfg flag).  Without a corrector that is
    the UNet's output, which the kernel combines; with one, `modify_score(model, e_t, x, t, c, **corrector_kwargs)` of the
    guidance-combined score (ddim.py:179-181, plms.py:188-190) -- a host callback, so such a run is eager."""
    r, b = run, run.b
    if score_corrector is None:
        plain = (r.eps.data_ptr(), 1 if r.cfg else 0)
        return lambda: plain
    assert model.parameterization == "eps"
    eps_c = torch.empty_like(r.img0)

    def corrected():
        e_t = r.eps[:b] if not r.cfg else r.eps[:b] + scale * (r.eps[b:] - r.eps[:b])
        tcur = t_buf[:b].clone()
        eps_c.copy_(score_corrector.modify_score(model, e_t, r.img.clone(), tcur, cond, **(corrector_kwargs or {})))
        return eps_c.data_ptr(), 0
    return corrected


def quantize_fixup(model, x_prev, pred_x0, a_prev):
    """quantize_denoised, in place after an update kernel: pred_x0 snapped to the first stage's codebook and x_prev moved to
    sqrt(a_prev) Q(pred_x0) + dir_xt + noise (ddim.py:194-202, plms.py:208-215)."""
    q = model._quantize_denoised(pred_x0)
    x_prev.add_(torch.sqrt(a_prev) * (q - pred_x0))
    pred_x0.copy_(q)


def log_step(index, log_every_t, n_run):
    """Whether the step that ends at index `index` of an `n_run`-step run goes into the intermediates."""
    return index % log_every_t == 0 or index == n_run - 1


def check_conditioning(model, conditioning, batch_size, required):
    """The `sample()` preamble: conditioning=None is an error (`required`: the caller's message) unless the model is
    unconditional, and a conditioning of another batch size gets the reference's warning."""
    if conditioning is None and getattr(model.model, "conditioning_key", "crossattn") is not None:
        raise L.LdmkError(required)
    ctx, cat = split_cond(model, conditioning)
    first = ctx if ctx is not None else cat
    if first is not None and first.shape[0] != batch_size:
        print(f"Warning: Got {first.shape[0]} conditionings but batch-size is {batch_size}")
