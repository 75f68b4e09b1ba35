"""GPU: `DPMSolverSampler(model).solver(...).sample(...)` (DPM_Solver) against the reference's recorded runs
(tests/golden/g27_dpm_methods*.npz, made by tools/make_golden_dpm_methods.py from the real reference), graph replay against eager
launches, the state the loop keeps on the float-time launch program, and its equality with `DPMSolverSampler.sample` where the two
overlap.

# Tolerance: DESIGN section 18's rule, as tests/test_dpm_gpu.py.  For each recorded run d = max |fp32 reference - float64 reference|
# over ALL of its latents (stored as `<tag>_d`), and the run is held to max(1.5e-4, 4 d), absolute and relative.  As recorded (|x|
# reaches ~390 on these weights; the thresholded runs stay within |x_T|max = 3.7, the sub-interval run within 17):
#   ss3_6 7.3e-4   ss3_4 8.5e-4   ss3_5 8.5e-4   ss2_5 1.0e-3   ssf2_6 7.9e-4   ss3_6_logSNR 4.9e-4   ss2_4_quadratic 1.0e-3
#   eps_ss3_6 8.5e-4   eps_ms2_5 8.5e-4   eps_ms3_6 7.9e-4   tay_ss3_6 7.3e-4   tay_ss2_4 8.5e-4   tay_ms2_5 9.2e-4   eps_tay_ss3_6 6.1e-4
#   cfg_ss3_6 1.8e-3   thr_ms2_5 1.5e-4   thr_cfg_ss3_6 1.5e-4   dz_ms2_5 9.8e-4   sub_ss2_4 1.5e-4   split_ss2_4 7.7e-4
# The thresholding scale s of every evaluation and sample is held to the same bound, relative.  Model times are held to equality.
# Every case prints its measured ratio to the bound (DESIGN section 24 records the worst)."""
import contextlib

import numpy as np
import pytest
import torch

from conftest import rnd
from dpm_methods_cases import RUNS, bound, load_goldens, solver_kw
from helpers import make_fr_model

pytestmark = pytest.mark.gpu

SPLIT = dict(ks=(32, 32), stride=(16, 16), vqf=4, patch_distributed_vq=True, tie_braker=False, clip_min_weight=0.01,
             clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
H, W_ = 48, 64
BF16X3_TAGS = ["ss3_6", "eps_ms2_5", "thr_ms2_5"]           # one singlestep, one eps-form and one thresholded run


@pytest.fixture(scope="module")
def fr():
    return make_fr_model(gain=0.25)


@pytest.fixture(scope="module")
def g():
    return load_goldens()


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


def _cond(m, labels=(1, 6)):
    lab = torch.tensor(labels, device="cuda")[:, None]
    return m.cond_stage_model.embedding(lab), m.cond_stage_model.uncond_embedding(torch.zeros_like(lab))


def _solver(m, g, tag, **over):
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    c, uc = _cond(m)
    kw = dict(solver_kw(tag, g), conditioning=c)
    if RUNS[tag][2]:
        kw.update(unconditional_guidance_scale=3.0, unconditional_conditioning=uc)
    kw.update(over)
    return DPMSolverSampler(m).solver(**kw)


def _start(tag):
    return rnd(232, 2, 3, H, W_).cuda() if tag.startswith("split") else rnd(231, 2, 3, 32, 32).cuda()


def _same(a, b):
    (xa, ia), (xb, ib) = a, b
    return (torch.equal(xa, xb) and len(ia["x_inter"]) == len(ib["x_inter"]) and all(torch.equal(p, q) for p, q in zip(ia["x_inter"], ib["x_inter"]))
            and torch.equal(ia["t_input"], ib["t_input"]) and all(torch.equal(p, q) for p, q in zip(ia.get("s", []), ib.get("s", []))))


def check_run(g, tag, out, inter):
    tol = bound(g, tag)
    ref = torch.from_numpy(g[tag + "_x_inter"])
    xi = torch.stack(inter["x_inter"]).float().cpu()
    assert xi.shape == ref.shape and torch.equal(out.cpu(), xi[-1])
    assert np.array_equal(inter["t_input"].cpu().numpy(), g[tag + "_t_input"]), "the model time of every evaluation"
    ratio = ((xi - ref).abs() / (tol + tol * ref.abs())).max().item()
    print(f"  {tag}: max |diff| vs the reference {(xi - ref).abs().max().item():.3e} (|ref| up to {ref.abs().max().item():.1f}, bound {tol:.3e}); "
          f"ratio to the bound {ratio:.3f}")
    torch.testing.assert_close(xi, ref, rtol=tol, atol=tol)
    if tag + "_s" in g:
        s, s_ref = torch.stack(inter["s"]).cpu(), torch.from_numpy(g[tag + "_s"])
        assert s.shape == s_ref.shape
        print(f"  {tag}: s {s_ref.min().item():.4g} .. {s_ref.max().item():.4g}, worst relative difference {((s - s_ref).abs() / s_ref).max().item():.3e}")
        torch.testing.assert_close(s, s_ref, rtol=tol, atol=0)
        max_val = float(g[tag + "_max_val"])
        assert bool(((s == max_val) == (s_ref == max_val)).all()), "the floor binds where it bound in the reference"
    else:
        assert "s" not in inter
    return ratio


def run_case(m, g, tag, **over):
    patch = tag.startswith("split")
    if patch:
        m.split_input_params = dict(SPLIT)
    try:
        return _solver(m, g, tag, **over).sample(_start(tag), intermediates=True, **RUNS[tag][1])
    finally:
        if patch:
            del m.split_input_params


# ------------------------------------------------------------------------------------------ every golden case
@pytest.mark.parametrize("tag", list(RUNS))
def test_sample_against_the_reference(fr, g, tag):
    """With the tile plans of a 16-sample job (`policy_batch=16`), as tests/test_dpm_gpu.py: F16X2."""
    from dsml_thesis_amd import lib as L
    out, inter = run_case(fr, g, tag, policy_batch=16)
    unet = fr.model.diffusion_model
    assert bool(unet.f16x2)
    if not tag.startswith("split"):
        pg = unet.program(4 if RUNS[tag][2] else 2, 32, 32, 1, 0, float_time=True)
        assert pg._dpm_methods_loops and not getattr(pg, "small_route", False) and "t_f32" in pg.inputs
        assert [c[2].compute for c in pg.calls if c[3] == "ldmk_igemm"].count(L.COMPUTE_F16X2) >= 40
    check_run(g, tag, out, inter)


@pytest.mark.parametrize("tag", BF16X3_TAGS)
def test_sample_against_the_reference_in_bf16x3(fr, x3, g, monkeypatch, tag):
    from dsml_thesis_amd import lib as L
    with arithmetic(fr, x3, monkeypatch, False) as m:
        out, inter = run_case(m, g, tag, policy_batch=16)
        unet = m.model.diffusion_model
        assert not unet.f16x2
        pg = unet.program(2, 32, 32, 1, 0, float_time=True)
        kinds = [c[2].compute for c in pg.calls if c[3] == "ldmk_igemm"]
        assert kinds.count(L.COMPUTE_BF16X3) >= 40 and L.COMPUTE_F16X2 not in kinds
    check_run(g, tag, out, inter)


# ------------------------------------------------------------------------------------------ graph, state
@pytest.mark.parametrize("tag", ["ss3_6", "thr_cfg_ss3_6"])
def test_graph_is_bitwise_eager_and_every_run_starts_clean(fr, g, tag):
    eager = run_case(fr, g, tag)
    solver = _solver(fr, g, tag, use_graph=True)
    x, kw = _start(tag), RUNS[tag][1]
    graph = solver.sample(x, intermediates=True, **kw)
    assert _same(eager, graph), "hipGraph replay must be bitwise identical to eager launches"
    unet = fr.model.diffusion_model
    pg = unet.program(4 if RUNS[tag][2] else 2, 32, 32, 1, 0, float_time=True)
    graphs = [st["graph"] for st in pg._dpm_methods_loops.values() if st["graph"] is not None]
    assert graphs
    assert _same(eager, solver.sample(x, intermediates=True, **kw)), "a second sample() on the same solver: the same bits"
    assert [st["graph"] for st in pg._dpm_methods_loops.values() if st["graph"] is not None] == graphs, "and the same captured graph"
    # a run of another length on the same program leaves other contents in keep / the ring and another step_idx behind
    other = solver.sample(x, intermediates=True, **dict(kw, steps=4))
    assert len(other[1]["x_inter"]) == 5 and not torch.equal(other[0], eager[0])
    assert _same(eager, solver.sample(x, intermediates=True, **kw)), "not disturbed by the cached state of another run"
    assert _same(eager, run_case(fr, g, tag)), "a second eager run starts clean"
    out = solver.sample(x, **kw)
    assert torch.is_tensor(out) and torch.equal(out, eager[0]), "without intermediates: the final latent alone"


def test_one_graph_replay_per_model_evaluation(fr, g, monkeypatch):
    tag = "dz_ms2_5"                                       # 5 steps + the denoise_to_zero evaluation
    solver = _solver(fr, g, tag, use_graph=True)
    x, kw = _start(tag), RUNS[tag][1]
    first = solver.sample(x, intermediates=True, **kw)
    pg = fr.model.diffusion_model.program(2, 32, 32, 1, 0, float_time=True)
    (st,) = [st for key, st in pg._dpm_methods_loops.items() if st["graph"] is not None and dict(key[2][:-1]).get("denoise_to_zero")]
    replays, replay = [], st["graph"].replay
    monkeypatch.setattr(st["graph"], "replay", lambda: (replays.append(1), replay())[1])
    again = solver.sample(x, intermediates=True, **kw)
    assert len(replays) == 6, "NFE replays of one captured graph, one more for the denoise_to_zero row; no eager step"
    assert _same(first, again)


@pytest.mark.parametrize("cfg", [False, True], ids=["cfg1", "cfg3"])
def test_multistep_x0_equals_the_sampler_bit_for_bit(fr, cfg):
    """solver(predict_x0=True).sample(method='multistep', order=2, steps=5) == DPMSolverSampler.sample(S=5) (the branch the two
    surfaces share runs the sampler's own loop), and neither disturbs the other."""
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    c, uc = _cond(fr)
    guide = dict(unconditional_guidance_scale=3.0, unconditional_conditioning=uc) if cfg else {}
    x = rnd(231, 2, 3, 32, 32).cuda()
    s = DPMSolverSampler(fr)
    ref, ri = s.sample(S=5, batch_size=2, shape=[3, 32, 32], conditioning=c, x_T=x, intermediates=True, use_graph=True, **guide)
    out, inter = s.solver(conditioning=c, predict_x0=True, use_graph=True, **guide).sample(x, steps=5, order=2, method="multistep", intermediates=True)
    assert torch.equal(out, ref) and all(torch.equal(p, q) for p, q in zip(inter["x_inter"], ri["x_inter"]))
    again, _ = s.sample(S=5, batch_size=2, shape=[3, 32, 32], conditioning=c, x_T=x, intermediates=True, use_graph=True, **guide)
    assert torch.equal(again, ref), "the sampler's loop is not disturbed by the solver's"
    out3 = s.solver(conditioning=c, predict_x0=True, **guide).sample(x, steps=6, order=3, method="multistep")
    ref3, _ = s.sample(S=6, batch_size=2, shape=[3, 32, 32], conditioning=c, x_T=x, order=3, **guide)
    assert torch.equal(out3, ref3), "order 3 with lower_order_final: 1, 2, 3, 3, 2, 1 in both"


def test_thresholding_is_inert_in_the_eps_form_until_denoise_to_zero(fr, g):
    """dpm_solver.py:386-408: the eps form never reaches the thresholding; denoise_to_zero_fn is data_prediction_fn, which does."""
    x, kw = _start("eps_ms2_5"), RUNS["eps_ms2_5"][1]
    plain = _solver(fr, g, "eps_ms2_5").sample(x, **kw)
    thr = _solver(fr, g, "eps_ms2_5", thresholding=True, max_val=2.0).sample(x, intermediates=True, **kw)
    assert torch.equal(plain, thr[0]) and "s" not in thr[1]
    out, inter = _solver(fr, g, "eps_ms2_5", thresholding=True, max_val=2.0).sample(x, intermediates=True, denoise_to_zero=True, **kw)
    assert torch.equal(inter["x_inter"][-2], plain) and len(inter["s"]) == 6 and float(out.abs().max()) <= 1.0
