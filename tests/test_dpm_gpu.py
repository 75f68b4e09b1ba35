"""GPU: `DPMSolverSampler` against the reference's recorded runs (tests/golden/g23_dpm*.npz, made by tools/make_golden_dpm.py from
the real reference), graph replay against eager launches, the state the loop keeps on the float-time launch program, and the
real-valued timestep through `UNetModel.forward`.

# Tolerance: DESIGN section 18's rule.  For each recorded run d = max |fp32 reference - float64 reference| over ALL of its latents
# (stored with the float64 twin as `<tag>_d`; the float64 twin also moves the model times by its own rounding, which is part of d),
# and the bound of that run's cases is max(1.5e-4, 4 d), absolute and relative.  As recorded (|x| reaches ~390 on these weights):
#   S5 2.4e-4 -> 9.8e-4     S5_cfg 5.2e-4 -> 2.1e-3     S6_o3 6.1e-4 -> 2.4e-3     S2 2.6e-4 -> 1.0e-3     S15 1.8e-4 -> 7.3e-4
#   S5_logSNR 2.3e-4 -> 9.2e-4     S5_quadratic 2.4e-4 -> 9.8e-4     S5_nolof 2.7e-4 -> 1.1e-3     split_S5 2.1e-4 -> 8.5e-4
# The order-3 run is recorded with lower_order_final=False: with it the reference itself raises when the order drops to 2 over a
# three-entry history (dpm_solver.py:773).  The schedule 1, 2, 3, 3, 2, 1 is run here and held to what it must share with that run.
# Measured ratios to the bound are printed by every case (DESIGN section 19 records the worst)."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

from conftest import golden, rnd
from helpers import make_fr_model
from oracle import ldm_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

SPLIT = dict(ks=(32, 32), stride=(16, 16), vqf=4, patch_distributed_vq=True, tie_braker=False, clip_min_weight=0.01,
             clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
H, W_ = 48, 64
# tag -> (fixture file, keywords of sample, guidance)
CASES = {
    "S5": ("g23_dpm.npz", dict(S=5), False),
    "S5_cfg": ("g23_dpm.npz", dict(S=5), True),
    "S6_o3": ("g23_dpm.npz", dict(S=6, order=3, lower_order_final=False), False),
    "S2": ("g23_dpm.npz", dict(S=2), False),
    "S15": ("g23_dpm_options.npz", dict(S=15), False),
    "S5_logSNR": ("g23_dpm_options.npz", dict(S=5, skip_type="logSNR"), False),
    "S5_quadratic": ("g23_dpm_options.npz", dict(S=5, skip_type="time_quadratic"), False),
    "S5_nolof": ("g23_dpm_options.npz", dict(S=5, lower_order_final=False), False),
}


@pytest.fixture(scope="module")
def fr():
    return make_fr_model(gain=0.25)


@pytest.fixture(scope="module")
def gold():
    return {f: dict(golden(f)) for f in ("g23_dpm.npz", "g23_dpm_options.npz", "g23_dpm_f64.npz")}


def bound(gold, tag):
    return max(1.5e-4, 4 * float(gold["g23_dpm_f64.npz"][tag + "_d"]))


def close(a, b, tol, what=""):
    a, b = a.float().cpu(), torch.as_tensor(np.asarray(b)).float()
    print(f"  {what}: max |diff| vs the reference {(a - b).abs().max().item():.3e} (|ref| up to {b.abs().max().item():.1f}, bound {tol:.3e})")
    torch.testing.assert_close(a, b, rtol=tol, atol=tol)


def _cond(m, labels=(1, 6)):
    lab = torch.tensor(labels, device="cuda")[:, None]
    return m.cond_stage_model.embedding(lab), m.cond_stage_model.uncond_embedding(torch.zeros_like(lab))


def _kw(m, cfg, **over):
    c, uc = _cond(m)
    kw = dict(batch_size=2, shape=[3, 32, 32], conditioning=c, x_T=rnd(231, 2, 3, 32, 32).cuda(), intermediates=True)
    if cfg:
        kw.update(unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    kw.update(over)
    return kw


def _same(a, b):
    (xa, ia), (xb, ib) = a, b
    return torch.equal(xa, xb) and len(ia["x_inter"]) == len(ib["x_inter"]) and all(torch.equal(p, q) for p, q in zip(ia["x_inter"], ib["x_inter"]))


def check_run(gold, tag, out, inter):
    fname, kw, _ = CASES[tag]
    g = gold[fname]
    xi = inter["x_inter"]
    assert len(xi) == kw["S"] + 1 and torch.equal(out, xi[-1])
    idx = [int(i) for i in g[tag + "_x_inter_idx"]]
    close(torch.stack([xi[i] for i in idx]), g[tag + "_x_inter"], bound(gold, tag), tag + " x_inter")


# ------------------------------------------------------------------------------------------ every golden case, both arithmetics
@pytest.fixture(scope="module")
def x3():
    holder = {}                                            # the bf16x3 model, built by the first case that asks for it
    yield holder
    holder.clear()


@contextlib.contextmanager
def arithmetic(fr, _X3, monkeypatch, f16x2):
    """The model in the asked arithmetic: the module's for F16X2; for bf16x3 one built (once) and run under LDMK_F16X2=0."""
    from dsml_thesis_amd import engine
    if f16x2:
        yield fr
        return
    monkeypatch.setenv("LDMK_F16X2", "0")
    engine.reset_tables()
    try:
        if "m" not in _X3:
            _X3["m"] = make_fr_model(gain=0.25)
        yield _X3["m"]
    finally:
        monkeypatch.delenv("LDMK_F16X2")
        engine.reset_tables()


@pytest.mark.parametrize("tag", list(CASES))
@pytest.mark.parametrize("f16x2", [True, False], ids=["f16x2", "bf16x3"])
def test_sample_against_the_reference(fr, x3, gold, monkeypatch, f16x2, tag):
    """With the tile plans of a 16-sample job (`policy_batch=16`): at its own batch of 2 this model runs the small-batch launch
    program, whose kernels are fp32 under either setting, and the two arms would be one."""
    from dsml_thesis_amd import lib as L
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    _, kw, cfg = CASES[tag]
    with arithmetic(fr, x3, monkeypatch, f16x2) as m:
        out, inter = DPMSolverSampler(m).sample(policy_batch=16, **_kw(m, cfg, **kw))
        unet = m.model.diffusion_model
        assert bool(unet.f16x2) == f16x2
        pg = unet.program(4 if cfg else 2, 32, 32, 1, 0, float_time=True)     # (policy_batch is still the run's)
        assert pg._dpm_loops and not getattr(pg, "small_route", False) and "t_f32" in pg.inputs
        kinds = [c[2].compute for c in pg.calls if c[3] == "ldmk_igemm"]
        assert kinds.count(L.COMPUTE_F16X2 if f16x2 else L.COMPUTE_BF16X3) >= 40 and (f16x2 or L.COMPUTE_F16X2 not in kinds)
    check_run(gold, tag, out, inter)


@pytest.mark.parametrize("f16x2", [True, False], ids=["f16x2", "bf16x3"])
def test_patch_wise(fr, x3, gold, monkeypatch, f16x2):
    """split_input_params at the 48x64 latent (Ly = 2, Lx = 3): unfold -> the float-time program at batch 12 -> fold around the same
    update; the advance fills all 12 entries of t_f32."""
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    g, b = gold["g23_dpm_options.npz"], bound(gold, "split_S5")
    with arithmetic(fr, x3, monkeypatch, f16x2) as m:
        c, _ = _cond(m)
        kw = dict(S=5, batch_size=2, shape=[3, H, W_], conditioning=c, x_T=rnd(232, 2, 3, H, W_).cuda(), intermediates=True, policy_batch=16)
        m.split_input_params = dict(SPLIT)
        try:
            s = DPMSolverSampler(m)
            out, inter = s.sample(**kw)
            assert [int(i) for i in g["split_S5_x_inter_idx"]] == [1, 5]
            close(torch.stack([inter["x_inter"][1], inter["x_inter"][5]]), g["split_S5_x_inter"], b, "patch-wise x_inter[1], [5]")
            if f16x2:
                assert _same((out, inter), s.sample(use_graph=True, **kw)) and _same((out, inter), s.sample(use_graph=True, **kw))
        finally:
            del m.split_input_params


def test_order_3_with_lower_order_final(fr, gold):
    """Orders 1, 2, 3, 3, 2, 1, which the reference cannot run: the first four steps are those of the recorded
    lower_order_final=False run bit for bit (the same table rows); the last two replace an order-3 update by an order-2 and an
    order-1 one over the same ring (tests/test_dpm_ops_gpu.py holds each order to its formula, tests/test_dpm_cpu.py the
    schedule), and the graphed run equals the eager one."""
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    s = DPMSolverSampler(fr)
    _, a = s.sample(**_kw(fr, False, S=6, order=3, lower_order_final=False))
    out, b = s.sample(**_kw(fr, False, S=6, order=3))
    assert all(torch.equal(p, q) for p, q in zip(a["x_inter"][:5], b["x_inter"][:5]))
    assert not torch.equal(a["x_inter"][5], b["x_inter"][5]) and torch.isfinite(out).all()
    assert _same((out, b), s.sample(use_graph=True, **_kw(fr, False, S=6, order=3)))


# ------------------------------------------------------------------------------------------ graph, state
@pytest.mark.parametrize("cfg", [False, True], ids=["cfg1", "cfg3"])
def test_graph_is_bitwise_eager_and_every_run_starts_clean(fr, cfg):
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    kw = _kw(fr, cfg, S=5)
    s = DPMSolverSampler(fr)
    eager = s.sample(**kw)
    graph = s.sample(use_graph=True, **kw)
    assert _same(eager, graph), "hipGraph replay must be bitwise identical to eager launches"
    assert _same(eager, s.sample(use_graph=True, **kw)), "a cached graph replays from a clean ring"
    assert _same(eager, s.sample(**kw)), "a second eager run starts from a clean ring"
    assert _same(eager, DPMSolverSampler(fr).sample(use_graph=True, **kw)), "a fresh sampler on the same program"
    # a run of another length and order in between leaves other contents in the ring and another step_idx behind
    s.sample(use_graph=True, **dict(kw, S=4, order=3))
    assert _same(eager, s.sample(use_graph=True, **kw))
    out, none = s.sample(use_graph=True, **dict(kw, intermediates=False))
    assert none is None and torch.equal(out, eager[0])


def test_one_unet_evaluation_per_step_and_one_graph_for_the_whole_run(fr, monkeypatch):
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    unet = fr.model.diffusion_model
    unet.policy_batch = None
    pg = unet.program(2, 32, 32, 1, 0, float_time=True)
    runs, run = [], pg.run

    def counted(*a, **k):
        runs.append(1)
        return run(*a, **k)
    monkeypatch.setattr(pg, "run", counted)
    DPMSolverSampler(fr).sample(**_kw(fr, False, S=5))
    assert len(runs) == 5, "one model evaluation per step, the first step included"
    monkeypatch.undo()
    s = DPMSolverSampler(fr)
    s.sample(use_graph=True, **_kw(fr, False, S=5))
    st = pg._dpm_loops[(False, 1.0, s._table_for(5, 2, "time_uniform", True).key, True)]      # (cfg, scale, table, graphed)
    assert st["graph"] is not None
    replays, replay = [], st["graph"].replay
    monkeypatch.setattr(st["graph"], "replay", lambda: (replays.append(1), replay())[1])
    s.sample(use_graph=True, **_kw(fr, False, S=5))
    assert len(replays) == 5, "S replays of one captured graph; no eager step"


def test_small_batch_route_at_batch_1(fr, gold):
    """Batch 1 takes the small-batch float-time program; a sample's trajectory is the first item of the recorded batch-2 run."""
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    c, _ = _cond(fr, labels=(1,))
    kw = dict(S=5, batch_size=1, shape=[3, 32, 32], conditioning=c, x_T=rnd(231, 2, 3, 32, 32)[:1].cuda(), intermediates=True)
    s = DPMSolverSampler(fr)
    out, inter = s.sample(**kw)
    pg = fr.model.diffusion_model.program(1, 32, 32, 1, 0, float_time=True)
    assert getattr(pg, "small_route", False) and pg._dpm_loops
    close(torch.stack(inter["x_inter"]), gold["g23_dpm.npz"]["S5_x_inter"][:, :1], bound(gold, "S5"), "batch 1, small route")
    assert _same((out, inter), s.sample(use_graph=True, **kw))


def test_ignored_keywords_change_no_bit(fr):
    """sampler.py:55-82 never passes them on."""
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    kw = _kw(fr, True, S=4)
    plain = DPMSolverSampler(fr).sample(**kw)
    calls = []
    other = DPMSolverSampler(fr).sample(mask=(rnd(5, 2, 1, 32, 32) > 0).float().cuda(), x0=rnd(6, 2, 3, 32, 32).cuda(), quantize_x0=True,
                                        eta=1.0, temperature=0.5, noise_dropout=0.3, score_corrector=object(), corrector_kwargs=dict(a=1),
                                        callback=calls.append, img_callback=lambda *a: calls.append(a), normals_sequence=[1],
                                        verbose=False, log_every_t=1, **kw)
    assert _same(plain, other) and not calls


def test_batch_size_warning(fr, capsys):
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    c, _ = _cond(fr, labels=(1, 6, 3))
    with pytest.raises(Exception):                         # (three conditionings for two latents cannot run; the warning comes first)
        DPMSolverSampler(fr).sample(S=2, batch_size=2, shape=[3, 32, 32], conditioning=c, x_T=rnd(231, 2, 3, 32, 32).cuda())
    assert "Warning: Got 3 conditionings but batch-size is 2" in capsys.readouterr().out


def test_ddim_is_untouched_by_a_dpm_run_on_the_same_model(fr):
    from dsml_thesis_amd.ddim import DDIMSampler
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    c, uc = _cond(fr)
    kw = dict(S=5, batch_size=2, shape=[3, 32, 32], conditioning=c, x_T=rnd(231, 2, 3, 32, 32).cuda(), use_graph=True,
              unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    before, _ = DDIMSampler(fr).sample(eta=0.0, verbose=False, **kw)
    dpm, _ = DPMSolverSampler(fr).sample(**kw)
    after, _ = DDIMSampler(fr).sample(eta=0.0, verbose=False, **kw)
    assert torch.equal(before, after) and not torch.equal(before, dpm)
    unet = fr.model.diffusion_model
    assert unet.program(4, 32, 32, 1, 0) is not unet.program(4, 32, 32, 1, 0, float_time=True)


def test_f16x2_range_fallback_inside_a_graphed_run():
    """As tests/test_sampling_gpu.py does it for DDIM: a checkpoint whose attn1.to_k weights of one block are 3000 x larger (to_q as
    much smaller: same logits) finishes its graphed run, the sampler reads the flags once, warns, re-plans THAT site in bf16x3 and
    repeats the run from a clean state -- bit for bit what a model that was told about the site up front samples."""
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    site = "input_blocks.1.1.transformer_blocks.0.attn1"

    def model():
        m = make_fr_model(gain=0.25)
        sd = m.model.diffusion_model.state_dict()
        key = site + ".to_k.weight"
        sd[key] = sd[key] * 3000.0
        sd[key.replace("to_k", "to_q")] = sd[key.replace("to_k", "to_q")] / 3000.0
        m.model.diffusion_model.load_state_dict(sd, strict=True)
        return m
    xT = rnd(52, 16, 3, 32, 32).cuda()
    m = model()
    c, _ = _cond(m, labels=tuple(i % 7 for i in range(16)))
    kw = dict(S=4, batch_size=16, shape=[3, 32, 32], conditioning=c, x_T=xT, intermediates=True)
    with pytest.warns(RuntimeWarning, match="F16X2"):
        out = DPMSolverSampler(m).sample(use_graph=True, **kw)
    st = m.model.diffusion_model.arithmetic_status()
    assert st["f16x2"] and st["denied"] == [site] and torch.isfinite(out[0]).all(), st
    m0 = model()
    m0.model.diffusion_model.deny_f16x2([site])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ref = DPMSolverSampler(m0).sample(use_graph=False, **kw)
    assert _same(out, ref)


# ------------------------------------------------------------------------------------------ the real-valued timestep in forward()
@pytest.mark.parametrize("route", ["small", "batched"])
def test_unet_forward_with_a_fractional_timestep(route):
    """timesteps = [799.2, 0.5] against the oracle (which embeds float timesteps as they are, util.py:161-165) at the UNet bound of
    tests/test_unet_gpu.py, 3e-5; the integer-valued float tensor [799., 0.] gives the bits of the int64 call."""
    from test_unet_gpu import make_unet
    m, sd = make_unet(W.FR_UNET)
    m.policy_batch = None if route == "small" else 16
    x, ctx = rnd(41, 2, 3, 32, 32), rnd(42, 2, 1, 512)
    t = torch.tensor([799.2, 0.5])
    eps = m(x.cuda(), t.cuda(), context=ctx.cuda())
    pg = m.program(2, 32, 32, 1, 0, float_time=True)
    assert bool(getattr(pg, "small_route", False)) == (route == "small")
    ref = O.unet_forward(sd, W.FR_UNET, x, t, ctx)
    trunc = O.unet_forward(sd, W.FR_UNET, x, t.to(torch.int64), ctx)
    print(f"  max |eps - oracle(799.2, 0.5)| {(eps.cpu() - ref).abs().max().item():.3e}; |oracle(799.2, 0.5) - oracle(799, 0)| "
          f"{(ref - trunc).abs().max().item():.3e}")
    torch.testing.assert_close(eps.cpu(), ref, rtol=3e-5, atol=3e-5)
    assert (ref - trunc).abs().max().item() > 3e-4, "the fixture tells a truncated timestep from the real one"
    ti = torch.tensor([799, 0])
    assert torch.equal(m(x.cuda(), ti.to(torch.float32).cuda(), context=ctx.cuda()), m(x.cuda(), ti.cuda(), context=ctx.cuda()))
    assert torch.equal(m(x.cuda(), ti.to(torch.float64).cuda(), context=ctx.cuda()), m(x.cuda(), ti.cuda(), context=ctx.cuda()))


def test_apply_model_with_a_fractional_timestep(fr):
    """LatentDiffusion.apply_model sends a floating-point t to the float-time program, plain and patch-wise."""
    c, _ = _cond(fr)
    x, t = rnd(231, 2, 3, 32, 32).cuda(), torch.tensor([799.2, 0.5]).cuda()
    unet = fr.model.diffusion_model
    unet.policy_batch = None
    e = fr.apply_model(x, t, c)
    assert torch.equal(e, unet(x, t, context=c)) and not torch.equal(e, fr.apply_model(x, t.long(), c))
    xs = rnd(232, 2, 3, H, W_).cuda()
    fr.split_input_params = dict(SPLIT)
    try:
        ef, ei = fr.apply_model(xs, t, c), fr.apply_model(xs, t.long(), c)
        assert torch.isfinite(ef).all() and not torch.equal(ef, ei)
        assert torch.equal(fr.apply_model(xs, t.long().float(), c), ei)
    finally:
        del fr.split_input_params
