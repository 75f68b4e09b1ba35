"""No GPU: the host side of the full diffusion objective (x0 / l1 / learned logvar / VLB) -- the VLB weights against the
reference's (tests/golden/g25_objective.npz, tools/make_golden_objective.py), the constructor's new arguments, where `logvar`
lives, which samplers refuse an x0-prediction model, and the new entry point's presence and argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(image_size=16, in_channels=3, out_channels=3, model_channels=32, attention_resolutions=[1], num_res_blocks=1,
             channel_mult=[1], num_head_channels=32, use_spatial_transformer=True, transformer_depth=1, context_dim=512)


def _model(cls=None, **kw):
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.ddpm import LatentDiffusion
    return (cls or LatentDiffusion)(**dict(synth.fr_config(unet=SMALL), **kw))


@pytest.mark.parametrize("case, par", [("a", "eps"), ("b", "x0")])
def test_lvlb_weights_match_the_reference(case, par):
    from dsml_thesis_amd import schedule as S, synth
    g = golden("g25_objective.npz")
    betas = S.make_beta_schedule("linear", synth.SCHEDULE["timesteps"], linear_start=synth.SCHEDULE["linear_start"],
                                 linear_end=synth.SCHEDULE["linear_end"])
    bufs = S.schedule_buffers(betas, 0.0, par)
    w, ref = bufs["lvlb_weights"], torch.from_numpy(g[f"{case}_lvlb_weights"])
    assert w.dtype == torch.float32 and w.shape == ref.shape == (1000,)
    assert torch.isfinite(w).all() and w[0] == w[1]
    torch.testing.assert_close(w, ref, rtol=1e-6, atol=0)
    assert "lvlb_weights" not in S.schedule_buffers(betas, 0.0)          # the existing callers' dictionary is what it was
    with pytest.raises(NotImplementedError):
        S.schedule_buffers(betas, 0.0, "mu")


def test_constructor_keeps_the_objective_settings_and_logvar_is_a_parameter_only_when_learned():
    m = _model(parameterization="x0", loss_type="l1", l_simple_weight=0.8, original_elbo_weight=10., learn_logvar=True, logvar_init=-0.7)
    assert (m.parameterization, m.loss_type, m.l_simple_weight, m.original_elbo_weight, m.learn_logvar) == ("x0", "l1", 0.8, 10., True)
    assert isinstance(m.logvar, torch.nn.Parameter) and m.logvar.shape == (1000,) and bool((m.logvar == -0.7).all())
    sd = m.state_dict()
    assert "logvar" in sd and "lvlb_weights" not in sd and not m._default_objective
    assert m.lvlb_weights.shape == (1000,)
    # a reference checkpoint of a learned-logvar run carries the key: it loads, strictly
    sd["logvar"] = torch.linspace(-1, 1, 1000)
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.logvar.data, sd["logvar"])
    assert m.to(torch.float64).logvar.dtype == torch.float64             # it follows .to(...) like any parameter

    fixed = _model(logvar_init=0.3)
    assert not isinstance(fixed.logvar, torch.nn.Parameter) and "logvar" not in fixed.state_dict() and not fixed._default_objective
    assert "lvlb_weights" not in fixed.state_dict()
    default = _model()
    assert default._default_objective and (default.loss_type, default.l_simple_weight, default.original_elbo_weight) == ("l2", 1., 0.)
    for kw in (dict(loss_type="l1"), dict(l_simple_weight=0.5), dict(original_elbo_weight=1.), dict(parameterization="x0"),
               dict(learn_logvar=True)):
        assert not _model(**kw)._default_objective, kw


def test_unknown_loss_type_or_parameterization_raise():
    with pytest.raises(NotImplementedError, match="unknown loss type"):
        _model(loss_type="huber")
    with pytest.raises(AssertionError, match="eps"):
        _model(parameterization="v")


def test_configure_optimizers_prints_the_reference_line(capsys):
    m = _model(learn_logvar=True)
    m.configure_optimizers()
    assert "Diffusion model optimizing logvar" in capsys.readouterr().out
    _model().configure_optimizers()
    assert "optimizing logvar" not in capsys.readouterr().out


def test_eps_samplers_and_fine_tunes_refuse_an_x0_model():
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.ddim import DDIMSampler
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    from dsml_thesis_amd.latent_diffclip import LatentDiffusionCLIP
    from dsml_thesis_amd.latent_tune import LatentDiffusionTune
    from dsml_thesis_amd.plms import PLMSSampler
    m = _model(parameterization="x0")
    for cls in (DDIMSampler, PLMSSampler, DPMSolverSampler):
        with pytest.raises(NotImplementedError, match="predicts 'x0'"):
            cls(m)
        cls(_model())                                                    # an eps model is taken as before
    with pytest.raises(NotImplementedError, match="predicts 'x0'"):
        _model(LatentDiffusionCLIP, parameterization="x0", edit_attr="happy")
    tf = synth.tf_config()
    tf["unet_config"] = dict(tf["unet_config"], params=dict(SMALL, in_channels=9, context_dim=1024))
    with pytest.raises(NotImplementedError, match="predicts 'x0'"):
        LatentDiffusionTune(**tf, parameterization="x0")


def test_x0_ancestral_tables_pass_the_network_output_through():
    """ldmk_ddpm_step forms x_recon = A x - B out from the first two table columns: A = 0, B = -1 under x0-prediction."""
    tab, _ = _model(parameterization="x0")._ddpm_device_tables()
    assert bool((tab[:, 0] == 0).all()) and bool((tab[:, 1] == -1).all())
    m = _model()
    tab, _ = m._ddpm_device_tables()
    assert torch.equal(tab[:, 0], m.sqrt_recip_alphas_cumprod) and torch.equal(tab[:, 1], m.sqrt_recipm1_alphas_cumprod)


def test_symbol_is_declared_bound_and_checks_its_arguments():
    from dsml_thesis_amd import lib as L
    header = open(os.path.join(ROOT, "include", "ldmk.h")).read()
    for name in ("ldmk_diffusion_loss", "ldmk_diffusion_loss_scratch_elems"):
        assert name + "(" in header and name in L._SIGS and name in L.EXPORTED
    lib = L.load()
    assert lib.ldmk_diffusion_loss_scratch_elems(3) >= 3 * 4 and lib.ldmk_diffusion_loss_scratch_elems(0) == 0
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)                                          # 16-byte aligned host memory: no launch may follow
    ok = dict(pred=p, target=p, t=p, logvar=p, lvlb=p, dpred=p, dlogvar=p, scalars=p, ls=p, n=2, c=3, hw=4, T=10, loss_type=2,
              lsw=1.0, oew=0.0, scratch=p, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ldmk_diffusion_loss(*[a[k] for k in ok])

    for bad in (dict(c=33), dict(c=0), dict(n=0), dict(n=-1), dict(hw=0), dict(T=0), dict(pred=None), dict(target=None), dict(t=None),
                dict(logvar=None), dict(lvlb=None), dict(scalars=None), dict(ls=None), dict(scratch=None), dict(loss_type=3),
                dict(n=65536)):
        assert call(**bad) == -1, bad
        assert b"ldmk_diffusion_loss" in lib.ldmk_last_error(), bad
    assert call(c=33) == -1 and b"33 channels" in lib.ldmk_last_error()


def test_wrapper_refuses_cpu_tensors():
    from dsml_thesis_amd import lib as L
    from dsml_thesis_amd import train_ops as T
    with pytest.raises(L.LdmkError):
        T.diffusion_loss(torch.zeros(1, 4, 32), torch.zeros(1, 3, 2, 2), torch.zeros(1, dtype=torch.int64), torch.zeros(10), torch.zeros(10))
