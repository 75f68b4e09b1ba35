"""PLMSSampler: drop-in for the reference's pseudo linear multistep sampler
  face_reenactment/ldm/models/diffusion/plms.py:11-236 (the talking-face tree carries an identical copy).

Same call surface (`make_schedule`, `sample`, `plms_sampling`, `p_sample_plms`).  Everything before the first step -- conditioning
split, guidance doubling, 'adm' labels, launch program or patch-wise evaluator, context program -- is `sampling_loop.prepare_run`
(through `DDIMSampler._prepare_run`), and the option handling, loop state and graph capture are that module's too; the loop differs
from DDIM's in two things.  The update is `ldmk_plms_step`: the DDIM update applied to an Adams-Bashforth combination of the
current and up to three past model outputs, which stay in a device ring next to a device count of how many are stored.  And the
first step evaluates the UNet twice (Euler predictor at t, corrector at t_next), so it runs as eager launches; steps 1 .. n-1 are one
captured graph (UNet program + one multistep launch) whose order follows the device count.  Additions over the reference:
`use_graph=`, `policy_batch=`, `mask_noise=`, as on `DDIMSampler`.
"""
import torch

from . import lib as L
from . import sampling_loop as SL
from .ddim import DDIMSampler
from .unet import rerun_if_flags_tripped


class PLMSSampler(DDIMSampler):
    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')                      # plms.py:25-26
        super().make_schedule(ddim_num_steps, ddim_discretize=ddim_discretize, ddim_eta=ddim_eta, verbose=verbose)

    @staticmethod
    def _no_original_steps(flag):
        if flag:
            raise L.LdmkError("PLMSSampler: use_original_steps / ddim_use_original_steps is not supported.  The reference reads "
                              "self.model.ddim_sigmas_for_original_num_steps (plms.py:197), which nothing defines, so it raises "
                              "AttributeError there: there is no reference behaviour to reproduce")

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None,
               img_callback=None, quantize_x0=False, eta=0., mask=None, x0=None, temperature=1.,
               noise_dropout=0., score_corrector=None, corrector_kwargs=None, verbose=True, x_T=None,
               log_every_t=100, unconditional_guidance_scale=1., unconditional_conditioning=None,
               use_graph=False, policy_batch=None, **kwargs):
        SL.check_conditioning(self.model, conditioning, batch_size,
                              "PLMSSampler.sample: conditioning is required (this model is cross-attention / concat conditioned).  "
                              "Only an unconditional LDM (cond_stage_config '__is_unconditional__') samples with conditioning=None")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C_, H, W_ = shape
        size = (batch_size, C_, H, W_)
        return self.plms_sampling(conditioning, size, callback=callback, img_callback=img_callback, quantize_denoised=quantize_x0,
                                  mask=mask, x0=x0, ddim_use_original_steps=False, noise_dropout=noise_dropout,
                                  temperature=temperature, score_corrector=score_corrector, corrector_kwargs=corrector_kwargs,
                                  x_T=x_T, log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                                  unconditional_conditioning=unconditional_conditioning, use_graph=use_graph,
                                  policy_batch=policy_batch, mask_noise=kwargs.get("mask_noise"))

    @torch.no_grad()
    def plms_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.,
                      noise_dropout=0., score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, use_graph=False, policy_batch=None, mask_noise=None):
        """plms.py:115-170.  `timesteps`: the first `int(min(timesteps / S, 1) S) - 1` entries of the DDIM subsequence (:130-132).
        The rarely used options run as they do in `DDIMSampler.ddim_sampling`, device-side around the same launches: mask / x0
        (+ `mask_noise`, one q_sample draw per step) blend before every step; quantize_denoised snaps pred_x0 to the codebook
        before x_prev is formed, in the Euler predictor too (the reference forms x_prev twice in step 0); score_corrector acts on
        every model output (two in step 0) and makes the run eager; temperature / noise_dropout scale a noise whose sigma is 0."""
        self._no_original_steps(ddim_use_original_steps)
        return self._plms_loop(cond, shape, x_T, callback, timesteps, quantize_denoised, mask, x0, img_callback, log_every_t,
                               score_corrector, corrector_kwargs, unconditional_guidance_scale, unconditional_conditioning, use_graph,
                               policy_batch, mask_noise)

    @rerun_if_flags_tripped(lambda self: self.model.model.diffusion_model)
    def _plms_loop(self, cond, shape, x_T, callback, timesteps, quantize_denoised, mask, x0, img_callback, log_every_t, score_corrector,
                   corrector_kwargs, unconditional_guidance_scale, unconditional_conditioning, use_graph, policy_batch, mask_noise):
        r = self._prepare_run(cond, shape, x_T, unconditional_guidance_scale, unconditional_conditioning, policy_batch, "plms")
        dev, b, img0, pg, img, run_net = r.dev, r.b, r.img0, r.pg, r.img, r.run_net
        S = self.ddim_timesteps.shape[0]
        lib = pg.lib
        t_buf = pg.inputs["t"]
        n_ts = t_buf.numel()
        if score_corrector is not None:
            use_graph = False                              # a host callback sits inside the step
        extras = mask is not None or quantize_denoised or score_corrector is not None
        table, ts_table, tsteps = self._table, self._ts_table, self.ddim_timesteps
        n_run = S if timesteps is None else int(min(timesteps / S, 1) * S) - 1
        assert 0 < n_run <= S, (n_run, S)
        use_graph = bool(use_graph) and n_run > 1          # (one step: the eager first step is the whole run)
        scale = float(unconditional_guidance_scale)
        # ring[k % 3] = the output of schedule index k; `count` = how many of them are stored (ldmk_plms_step)
        st = r.state((r.cfg, scale, self._sched_key, use_graph, n_run), lambda: dict(
            pred_x0=torch.empty_like(img0), keep=torch.empty_like(img0), ring=torch.empty((3,) + tuple(img0.shape), device=dev),
            step_idx=torch.zeros(1, dtype=torch.int32, device=dev), count=torch.zeros(1, dtype=torch.int32, device=dev)),
            cached=not extras)
        pred_x0, keep, ring, step_idx, count = st["pred_x0"], st["keep"], st["ring"], st["step_idx"], st["count"]
        per = img0[0].numel()
        blend = SL.MaskBlend(r, self.model, mask, x0, mask_noise) if mask is not None else None
        score = SL.score_source(r, self.model, score_corrector, corrector_kwargs, cond, scale, t_buf)

        def reset_state():
            r.seed()
            step_idx.fill_(n_run - 1)
            count.zero_()                                  # the ring's contents are dead without it
            t_buf.fill_(int(tsteps[n_run - 1]))

        def update(mode, x_in):
            """The model output in `eps` -> one ldmk_plms_step launch (+ advance) -> the quantisation fix-up."""
            a_prev = table[step_idx.long(), 1] if quantize_denoised else None      # read before the kernel advances the counter
            e_ptr, k_cfg = score()
            rc = lib.ldmk_plms_step(x_in.data_ptr(), e_ptr, table.data_ptr(), step_idx.data_ptr(), count.data_ptr(), scale, k_cfg,
                                    mode, ring.data_ptr(), keep.data_ptr() if mode == L.PLMS_PREDICTOR else 0, img.data_ptr(),
                                    pred_x0.data_ptr(), per, b, ts_table.data_ptr(), t_buf.data_ptr(), n_ts, 1, S,
                                    torch.cuda.current_stream().cuda_stream)
            L.check(rc, "ldmk_plms_step")
            if quantize_denoised:
                SL.quantize_fixup(self.model, img, pred_x0, a_prev)
            r.share_latent()

        def first_step():                                  # two UNet evaluations (plms.py:219-223): eager launches
            if blend is not None:
                blend.blend(t_buf)
            run_net()
            update(L.PLMS_PREDICTOR, img)                  # img <- the Euler prediction, keep <- img, t <- t_next
            run_net()
            update(L.PLMS_CORRECTOR, keep)

        def multistep():
            if blend is not None:
                blend.blend(t_buf)
            run_net()
            update(L.PLMS_MULTISTEP, img)

        reset_state()
        step = r.stepper(st, multistep, reset_state, use_graph, blend.draw if blend is not None else None)
        intermediates = {"x_inter": [img0], "pred_x0": [img0]}
        for i in range(n_run):
            if blend is not None:
                blend.feed(i)
                if i == 0 or not use_graph:                # (the first step is eager; a captured multistep draws inside)
                    blend.draw()
            if i == 0:
                first_step()
            else:
                step()
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            if SL.log_step(n_run - i - 1, log_every_t, n_run):
                intermediates["x_inter"].append(img.clone())
                intermediates["pred_x0"].append(pred_x0.clone())
        return img.clone(), intermediates

    @torch.no_grad()
    def p_sample_plms(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, old_eps=None, t_next=None):
        """Single step with the reference's signature (plms.py:173-236); returns (x_prev, pred_x0, e_t).  `old_eps`: the caller's
        list of past outputs, newest last; empty (or None) takes the Euler branch, which evaluates the model again at `t_next`."""
        self._no_original_steps(use_original_steps)
        dev, b, index = x.device, x.shape[0], int(index)
        old_eps = [] if old_eps is None else list(old_eps)
        x = x.contiguous()
        table = self._table
        step_idx = torch.full((1,), index, dtype=torch.int32, device=dev)
        count = torch.full((1,), min(len(old_eps), 3), dtype=torch.int32, device=dev)
        ring = torch.zeros((3,) + tuple(x.shape), device=dev)
        for j, e_old in enumerate(reversed(old_eps[-3:]), start=1):             # old_eps[-j] = the output of index + j
            ring[(index + j) % 3].copy_(e_old)
        x_prev, pred_x0 = torch.empty_like(x), torch.empty_like(x)
        scale = float(unconditional_guidance_scale)

        def update(mode, x_in, x_at, t_at):
            e, cfg = self._model_output(x_at, c, t_at, unconditional_guidance_scale, unconditional_conditioning, score_corrector,
                                        corrector_kwargs)
            e = e.contiguous()
            L.call("ldmk_plms_step", x_in.data_ptr(), e.data_ptr(), table.data_ptr(), step_idx.data_ptr(), count.data_ptr(),
                   scale, 1 if cfg else 0, mode, ring.data_ptr(), 0, x_prev.data_ptr(), pred_x0.data_ptr(), x[0].numel(), b, 0, 0, 0, 0, 0,
                   torch.cuda.current_stream().cuda_stream)
            if quantize_denoised:                                               # plms.py:208-209
                SL.quantize_fixup(self.model, x_prev, pred_x0, table[index, 1])

        if old_eps:
            update(L.PLMS_MULTISTEP, x, x, t)
        else:
            update(L.PLMS_PREDICTOR, x, x, t)
            update(L.PLMS_CORRECTOR, x, x_prev.clone(), t_next)
        return x_prev, pred_x0, ring[index % 3].clone()
