"""GPU: `PLMSSampler` against the reference's recorded runs (tests/golden/g22_plms*.npz, made by tools/make_golden_plms.py from the
real reference classes), graph replay against eager launches, and the state the loop keeps on the launch program.

# Tolerance.  DDIM's 1.5e-4 is not reused blindly: the order-4 combination multiplies an error in eps by up to
# (55 + 59 + 37 + 9) / 24 = 6.7.  The reference is measured against itself: for each recorded run d = max |fp32 reference - float64
# reference| over its x_inter / pred_x0 arrays (the `*_f64` twins), and the bound for that run's cases is max(1.5e-4, 4 d), absolute
# and relative -- 4 for the split arithmetic's documented 1.0-1.7 x of an fp32 product's error and for the spread between RMS and
# max.  As recorded:   S = 5 guidance 1: d = 2.1e-5 -> 1.5e-4      S = 5 guidance 3: d = 8.9e-5 -> 3.5e-4
#                      S = 4 guidance 1: d = 1.1e-5 -> 1.5e-4      S = 4 guidance 3: d = 3.1e-5 -> 1.5e-4
# (the test recomputes them from the arrays).  Cases without a float64 twin (options, patch-wise, single steps) take the bound of the
# plain run with the same S and guidance.  The option cases run at S = 4 because the reference has no S = 3 (its uniform
# discretisation gives 1, 334, 667, 1000 and indexes alphas_cumprod[1000]).
"""
import contextlib

import numpy as np
import pytest
import torch

from conftest import golden, rnd
from helpers import make_fr_model

pytestmark = pytest.mark.gpu

SPLIT = dict(ks=(32, 32), stride=(16, 16), vqf=4, patch_distributed_vq=True, tie_braker=False, clip_min_weight=0.01,
             clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
H, W_ = 48, 64


@pytest.fixture(scope="module")
def fr():
    return make_fr_model(gain=0.25)


@pytest.fixture(scope="module")
def g22():
    return dict(golden("g22_plms.npz"))


@pytest.fixture(scope="module")
def gopt():
    return dict(golden("g22_plms_options.npz"))


@pytest.fixture(scope="module")
def bounds(g22, gopt):
    """max(1.5e-4, 4 d) per plain run, d from the float64 twins"""
    g64 = golden("g22_plms_f64.npz")
    out = {}
    for tag, src, keys in (("sample_S5", g22, ("_x_inter", "_pred_x0")), ("sample_S5_cfg", g22, ("_x_inter", "_pred_x0")),
                           ("sample_S4", gopt, ("", "_pred_x0")), ("sample_S4_cfg", gopt, ("", "_pred_x0"))):
        d = max(float(np.abs(src[tag + k].astype(np.float64) - g64[tag + k + "_f64"].astype(np.float64)).max()) for k in keys)
        out[tag] = max(1.5e-4, 4 * d)
        print(f"{tag}: d = {d:.3e}, bound {out[tag]:.3e}")
    return out


def close(a, b, tol, what=""):
    a, b = a.float().cpu(), torch.as_tensor(np.asarray(b)).float()
    print(f"  {what}: max |diff| vs the reference {(a - b).abs().max().item():.3e} (|ref| up to {b.abs().max().item():.1f}, bound {tol:.3e})")
    torch.testing.assert_close(a, b, rtol=tol, atol=tol)


def _cond(m, labels=(1, 6)):
    lab = torch.tensor(labels, device="cuda")[:, None]
    return m.cond_stage_model.embedding(lab), m.cond_stage_model.uncond_embedding(torch.zeros_like(lab))


def _kw(m, cfg, **over):
    c, uc = _cond(m)
    kw = dict(batch_size=2, shape=[3, 32, 32], conditioning=c, eta=0.0, x_T=rnd(221, 2, 3, 32, 32).cuda(), verbose=False)
    if cfg:
        kw.update(unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    kw.update(over)
    return kw


def _same(a, b):
    (xa, ia), (xb, ib) = a, b
    return torch.equal(xa, xb) and all(len(ia[k]) == len(ib[k]) and all(torch.equal(p, q) for p, q in zip(ia[k], ib[k])) for k in ia)


# ------------------------------------------------------------------------------------------ the S = 5 runs, both arithmetics
@pytest.mark.parametrize("cfg", [False, True], ids=["cfg1", "cfg3"])
@pytest.mark.parametrize("f16x2", [True, False], ids=["f16x2", "bf16x3"])
def test_sample_S5_against_the_reference(fr, g22, bounds, monkeypatch, f16x2, cfg):
    """Euler, order 2, order 3, order 4 with a full ring, order 4 after the ring has wrapped: every x_inter and pred_x0.  With the
    tile plans of a 16-sample job (`policy_batch=16`): at its own batch of 2 this model runs the small-batch launch program, whose
    kernels are fp32 under either setting, and the two arms would be one."""
    from dsml_thesis_amd import engine
    from dsml_thesis_amd import lib as L
    from dsml_thesis_amd.plms import PLMSSampler
    tag = "sample_S5_cfg" if cfg else "sample_S5"
    m = fr
    if not f16x2:
        monkeypatch.setenv("LDMK_F16X2", "0")
        engine.reset_tables()
    try:
        if not f16x2:
            m = make_fr_model(gain=0.25)
        out, inter = PLMSSampler(m).sample(S=5, log_every_t=1, policy_batch=16, **_kw(m, cfg))
        unet = m.model.diffusion_model
        assert bool(unet.f16x2) == f16x2
        pg = unet.program(4 if cfg else 2, 32, 32, 1, 0)                      # (policy_batch is still the run's)
        assert pg._plms_loops and not getattr(pg, "small_route", False)
        kinds = [c[2].compute for c in pg.calls if c[3] == "ldmk_igemm"]
        assert kinds.count(L.COMPUTE_F16X2 if f16x2 else L.COMPUTE_BF16X3) >= 40 and (f16x2 or L.COMPUTE_F16X2 not in kinds)
    finally:
        if not f16x2:
            monkeypatch.delenv("LDMK_F16X2")
            engine.reset_tables()
    assert len(inter["x_inter"]) == len(inter["pred_x0"]) == 6
    close(torch.stack(inter["x_inter"]), g22[tag + "_x_inter"], bounds[tag], tag + " x_inter")
    close(torch.stack(inter["pred_x0"]), g22[tag + "_pred_x0"], bounds[tag], tag + " pred_x0")
    assert torch.equal(out, inter["x_inter"][-1])


# ------------------------------------------------------------------------------------------ graph, state
@pytest.mark.parametrize("cfg", [False, True], ids=["cfg1", "cfg3"])
def test_graph_is_bitwise_eager_and_every_run_starts_clean(fr, cfg):
    from dsml_thesis_amd.plms import PLMSSampler
    kw = _kw(fr, cfg, S=5, log_every_t=1)
    s = PLMSSampler(fr)
    eager = s.sample(**kw)
    graph = s.sample(use_graph=True, **kw)
    assert _same(eager, graph), "hipGraph replay must be bitwise identical to eager launches"
    assert _same(eager, s.sample(use_graph=True, **kw)), "a cached graph replays from a clean ring"
    assert _same(eager, s.sample(**kw)), "a second eager run starts from a clean ring"
    assert _same(eager, PLMSSampler(fr).sample(use_graph=True, **kw)), "a fresh sampler on the same program"
    # a run of another length in between leaves other contents in the ring
    s.sample(use_graph=True, **dict(kw, S=4))
    assert _same(eager, s.sample(use_graph=True, **kw))


def test_intermediates_and_callbacks(fr, g22, bounds):
    """plms.py:134,163-168: x_T first, then the steps whose index is a multiple of log_every_t and the first step; callback(i),
    img_callback(pred_x0, i) after every step."""
    from dsml_thesis_amd.plms import PLMSSampler
    calls, seen = [], []
    out, inter = PLMSSampler(fr).sample(S=5, log_every_t=2, callback=calls.append,
                                        img_callback=lambda p, i: seen.append((i, p.clone())), **_kw(fr, False))
    assert calls == [0, 1, 2, 3, 4] and [i for i, _ in seen] == calls
    assert len(inter["x_inter"]) == len(inter["pred_x0"]) == 4             # x_T, index 4 (the first step), 2, 0
    assert torch.equal(inter["x_inter"][0].cpu(), rnd(221, 2, 3, 32, 32))
    b = bounds["sample_S5"]
    for mine, k in zip(inter["x_inter"][1:], (1, 3, 5)):
        close(mine, g22["sample_S5_x_inter"][k], b, f"x_inter entry of step {k - 1}")
    for mine, k in zip(inter["pred_x0"][1:], (1, 3, 5)):
        close(mine, g22["sample_S5_pred_x0"][k], b, f"pred_x0 entry of step {k - 1}")
    for i, p in seen:
        close(p, g22["sample_S5_pred_x0"][i + 1], b, f"img_callback {i}")
    out100, inter100 = PLMSSampler(fr).sample(S=5, **_kw(fr, False))         # log_every_t = 100: the first step and index 0
    assert len(inter100["x_inter"]) == 3 and torch.equal(out100, out)


def test_six_unet_evaluations_for_five_steps(fr, monkeypatch):
    from dsml_thesis_amd.plms import PLMSSampler
    fr.model.diffusion_model.policy_batch = None                             # (the plans of this batch, as the run below asks for)
    pg = fr.model.diffusion_model.program(2, 32, 32, 1, 0)
    runs, run = [], pg.run

    def counted(*a, **k):
        runs.append(1)
        return run(*a, **k)
    monkeypatch.setattr(pg, "run", counted)
    PLMSSampler(fr).sample(S=5, **_kw(fr, False))
    assert len(runs) == 6, "the first step evaluates the UNet twice, every other step once"


def test_ddim_is_untouched_by_a_plms_run_on_the_same_program(fr):
    from dsml_thesis_amd.ddim import DDIMSampler
    from dsml_thesis_amd.plms import PLMSSampler
    kw = _kw(fr, True, S=5, use_graph=True)
    before, _ = DDIMSampler(fr).sample(**kw)
    plms, _ = PLMSSampler(fr).sample(**kw)
    after, _ = DDIMSampler(fr).sample(**kw)
    assert torch.equal(before, after) and not torch.equal(before, plms)
    pg = fr.model.diffusion_model.program(4, 32, 32, 1, 0)
    assert pg._ddim_loops and pg._plms_loops and pg._ddim_loops is not pg._plms_loops


# ------------------------------------------------------------------------------------------ single steps
@pytest.mark.parametrize("n_old", [0, 1, 2, 3])
def test_p_sample_plms_with_a_hand_built_history(fr, gopt, bounds, n_old):
    from dsml_thesis_amd.plms import PLMSSampler
    c, uc = _cond(fr)
    s = PLMSSampler(fr)
    s.make_schedule(ddim_num_steps=5, ddim_eta=0.0, verbose=False)
    x = rnd(222, 2, 3, 32, 32).cuda()
    old = [(0.9 * rnd(223 + j, 2, 3, 32, 32)).cuda() for j in range(3)]
    index = 3
    t = torch.full((2,), int(s.ddim_timesteps[index]), device="cuda", dtype=torch.long)
    t_next = torch.full((2,), int(s.ddim_timesteps[index - 1]), device="cuda", dtype=torch.long)
    outs = s.p_sample_plms(x, c, t, index=index, old_eps=old[3 - n_old:], t_next=t_next, unconditional_guidance_scale=3.0,
                           unconditional_conditioning=uc)
    assert len(outs) == 3
    for mine, ref, name in zip(outs, gopt[f"p_sample_n{n_old}"], ("x_prev", "pred_x0", "e_t")):
        close(mine, ref, bounds["sample_S5_cfg"], f"{n_old} past outputs, {name}")


# ------------------------------------------------------------------------------------------ subset, options, patch-wise
def test_timesteps_subset(fr, g22, bounds):
    from dsml_thesis_amd.plms import PLMSSampler
    c, _ = _cond(fr)
    s = PLMSSampler(fr)
    s.make_schedule(ddim_num_steps=5, ddim_eta=0.0, verbose=False)
    xT = rnd(221, 2, 3, 32, 32).cuda()
    out, inter = s.plms_sampling(c, (2, 3, 32, 32), x_T=xT, timesteps=3, log_every_t=1)
    assert len(inter["x_inter"]) == 3                                         # int(min(3 / 5, 1) 5) - 1 = 2 steps
    close(torch.stack(inter["x_inter"]), g22["subset_S5_t3_x_inter"], bounds["sample_S5"], "subset x_inter")
    close(torch.stack(inter["pred_x0"]), g22["subset_S5_t3_pred_x0"], bounds["sample_S5"], "subset pred_x0")
    out_g, _ = s.plms_sampling(c, (2, 3, 32, 32), x_T=xT, timesteps=3, log_every_t=1, use_graph=True)
    assert torch.equal(out, out_g)


def test_plain_S4_runs(fr, gopt, bounds):
    from dsml_thesis_amd.plms import PLMSSampler
    for cfg, tag in ((False, "sample_S4"), (True, "sample_S4_cfg")):
        out, inter = PLMSSampler(fr).sample(S=4, log_every_t=1, **_kw(fr, cfg))
        close(out, gopt[tag], bounds[tag], tag)
        close(inter["pred_x0"][-1], gopt[tag + "_pred_x0"], bounds[tag], tag + " pred_x0")


def test_quantize_x0(fr, gopt, bounds):
    """pred_x0 snapped to the codebook before x_prev is formed, in the Euler predictor too."""
    from dsml_thesis_amd.plms import PLMSSampler
    out, inter = PLMSSampler(fr).sample(S=4, log_every_t=1, quantize_x0=True, **_kw(fr, False))
    close(out, gopt["quantize_S4"], bounds["sample_S4"], "quantize_x0")
    close(inter["pred_x0"][-1], gopt["quantize_S4_pred_x0"], bounds["sample_S4"], "quantize_x0 pred_x0")
    out_g, _ = PLMSSampler(fr).sample(S=4, log_every_t=1, quantize_x0=True, use_graph=True, **_kw(fr, False))
    assert torch.equal(out, out_g)


def test_mask_and_x0(fr, gopt, bounds):
    from dsml_thesis_amd.plms import PLMSSampler
    x0, mask = (0.5 * rnd(226, 2, 3, 32, 32)).cuda(), (rnd(227, 2, 1, 32, 32) > 0).float().cuda()
    kw = _kw(fr, True, S=4, log_every_t=1, mask=mask, x0=x0, mask_noise=torch.from_numpy(gopt["mask_noise"]).cuda())
    out, inter = PLMSSampler(fr).sample(**kw)
    close(out, gopt["mask_S4_cfg"], bounds["sample_S4_cfg"], "mask + x0")
    close(inter["pred_x0"][-1], gopt["mask_S4_cfg_pred_x0"], bounds["sample_S4_cfg"], "mask + x0 pred_x0")
    out_g, _ = PLMSSampler(fr).sample(use_graph=True, **kw)
    assert torch.equal(out, out_g), "the blend is device-side work: hipGraph replay == eager"


class _ShiftCorrector:
    """the deterministic stand-in tools/make_golden.py uses for the (unshipped) score-corrector plugin"""

    def __init__(self):
        self.calls = 0

    def modify_score(self, model, e_t, x, t, c, strength=0.1):
        self.calls += 1
        return e_t - strength * x * (t.float().view(-1, 1, 1, 1) / 1000.0)


def test_score_corrector(fr, gopt, bounds):
    from dsml_thesis_amd.plms import PLMSSampler
    corr = _ShiftCorrector()
    out, inter = PLMSSampler(fr).sample(S=4, log_every_t=1, score_corrector=corr, corrector_kwargs=dict(strength=0.2), use_graph=True,
                                        **_kw(fr, True))
    assert corr.calls == 5, "on every model output: twice in the first step"
    close(out, gopt["corrector_S4_cfg"], bounds["sample_S4_cfg"], "score_corrector")
    close(inter["pred_x0"][-1], gopt["corrector_S4_cfg_pred_x0"], bounds["sample_S4_cfg"], "score_corrector pred_x0")


@contextlib.contextmanager
def split(m):
    m.split_input_params = dict(SPLIT)
    try:
        yield m
    finally:
        del m.split_input_params


def test_patch_wise(fr, gopt, bounds):
    """split_input_params: unfold -> program -> fold around the same update, at the 48x64 latent (Ly = 2, Lx = 3)."""
    from dsml_thesis_amd.plms import PLMSSampler
    c, _ = _cond(fr)
    kw = dict(S=4, batch_size=2, shape=[3, H, W_], conditioning=c, eta=0.0, x_T=rnd(228, 2, 3, H, W_).cuda(), verbose=False)
    with split(fr):
        s = PLMSSampler(fr)
        out, _ = s.sample(**kw)
        close(out, gopt["split_S4"], bounds["sample_S4"], "patch-wise")
        out_g, _ = s.sample(use_graph=True, **kw)
        assert torch.equal(out, out_g)
        assert torch.equal(out, s.sample(use_graph=True, **kw)[0])


# ------------------------------------------------------------------------------------------ every conditioning key
def _models():
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.ddim import C12, C34
    from dsml_thesis_amd.ddpm import LatentDiffusion
    from helpers import make_tf_model, make_uncond_model

    def concat():
        cfg = synth.uncond_config(dict(synth.UNCOND_UNET, image_size=32, in_channels=7, out_channels=4), synth.VQ_F4_256)
        cfg.update(conditioning_key="concat", cond_stage_config="__is_first_stage__", channels=4, image_size=32)
        m = LatentDiffusion(**cfg)
        synth.load_recipe(m.model.diffusion_model, gain=0.25)
        return (m.cuda().eval(), [4, 32, 32], rnd(143, 2, 3, 32, 32).cuda(),
                dict(unconditional_guidance_scale=3.0, unconditional_conditioning=rnd(144, 2, 3, 32, 32).cuda()))

    def adm():
        from oracle import weights as W
        cfg = synth.fr_config(unet=W.UPDOWN_ADM_UNET)
        cfg.update(conditioning_key="adm")
        m = LatentDiffusion(**cfg)
        synth.load_recipe(m.model.diffusion_model, gain=0.25)
        return (m.cuda().eval(), [3, 16, 16], torch.tensor([7, 2]).cuda(),
                dict(unconditional_guidance_scale=3.0, unconditional_conditioning=torch.tensor([0, 0]).cuda()))

    def none():
        return make_uncond_model(gain=0.25), [4, 64, 64], None, {}

    def hybrid():
        return (make_tf_model(gain=0.25, seq_len=3), [3, 32, 32],
                {C12: rnd(145, 2, 1, 1024).cuda(), C34: rnd(146, 2, 6, 32, 32).cuda()}, {})
    return dict(concat=concat, adm=adm, none=none, hybrid=hybrid)


@pytest.mark.parametrize("key", ["concat", "adm", "none", "hybrid"])
def test_every_conditioning_key_of_the_ddim_loop(key):
    """None / concat / hybrid / adm (crossattn is every other test of this file), with guidance where the key has an unconditional
    form: the device-resident loop, eager and graphed, equals the chain of `p_sample_plms` single steps fed the history the
    reference's loop would keep -- bit for bit, as both run the same launch program and the same update kernel."""
    from dsml_thesis_amd.plms import PLMSSampler
    m, shape, cond, guide = _models()[key]()
    n = 4
    xT = rnd(147, 2, *shape).cuda()
    s = PLMSSampler(m)
    out, _ = s.sample(S=n, batch_size=2, shape=shape, conditioning=cond, eta=0.0, x_T=xT, verbose=False, **guide)
    out_g, _ = s.sample(S=n, batch_size=2, shape=shape, conditioning=cond, eta=0.0, x_T=xT, verbose=False, use_graph=True, **guide)
    assert torch.isfinite(out).all() and torch.equal(out, out_g)
    img, old = xT, []
    for i in range(n):
        index = n - 1 - i
        t = torch.full((2,), int(s.ddim_timesteps[index]), device="cuda", dtype=torch.long)
        t_next = torch.full((2,), int(s.ddim_timesteps[max(index - 1, 0)]), device="cuda", dtype=torch.long)
        img, _, e_t = s.p_sample_plms(img, cond, t, index=index, old_eps=old, t_next=t_next, **guide)
        old = (old + [e_t])[-3:]
    assert torch.equal(img, out), f"max |chain - loop| {(img - out).abs().max().item():.3e}"


# ------------------------------------------------------------------------------------------ refusals on the device path
def test_refusals(fr):
    from dsml_thesis_amd.lib import LdmkError
    from dsml_thesis_amd.plms import PLMSSampler
    s = PLMSSampler(fr)
    with pytest.raises(ValueError, match="ddim_eta must be 0 for PLMS"):
        s.sample(S=5, **dict(_kw(fr, False), eta=1.0))
    with pytest.raises(LdmkError, match="conditioning is required"):
        s.sample(S=5, **dict(_kw(fr, False), conditioning=None))
