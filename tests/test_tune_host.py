"""CPU: the host side of the talking-face lip-reading fine-tune (ddpm2condtune.py): the fourth shipped YAML resolves to
`LatentDiffusionTune`, the 8-step eta = 1 coefficient rows, and the loss-weight switch."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden


def _strip_ckpt(node):
    if isinstance(node, dict):
        return {k: _strip_ckpt(v) for k, v in node.items() if k != "ckpt_path"}
    if isinstance(node, list):
        return [_strip_ckpt(v) for v in node]
    return node


@pytest.fixture(scope="module")
def tune_model():
    from dsml_thesis_amd.util import instantiate_from_config, load_yaml_config
    cfg = _strip_ckpt(load_yaml_config(os.path.join(GOLDEN, "configs", "mead-128-ldm-f4-tune.yaml")))["model"]
    assert cfg["target"] == "ldm.models.diffusion.ddpm2condtune.LatentDiffusion"
    return instantiate_from_config(cfg), cfg


def test_shipped_tune_yaml_instantiates_latent_diffusion_tune(tune_model):
    """talking_face/configs/latent-diffusion/mead-128-ldm-f4-tune.yaml, unchanged, through the `target:` factory."""
    from dsml_thesis_amd.ddpm import LatentDiffusion2Cond
    from dsml_thesis_amd.latent_tune import LatentDiffusionTune
    model, cfg = tune_model
    assert type(model) is LatentDiffusionTune and isinstance(model, LatentDiffusion2Cond)
    p = cfg["params"]
    assert model.lr_loss_w == p["lr_loss_w"] == 1.0 and model.start_lr_loss == p["start_lr_loss"] == 0
    assert model.num_tune_steps == 8 and model.tune_eta == 1.0                    # make_schedule(8, ddim_eta=1.0)
    assert model.lip_loss_func is None and model.cond_stage_trainable and model.concat_mode is False
    assert model.model.conditioning_key == "crossattn"
    assert model.cond_stage_model_2.seq_len == 9 and model.model.diffusion_model.in_channels == 9
    assert model.num_timesteps == 1000 and model.channels == 3 and model.image_size == 32


def test_constructor_asserts_what_the_reference_asserts(tune_model):
    from dsml_thesis_amd.latent_tune import LatentDiffusionTune
    _, cfg = tune_model
    small = dict(cfg["params"])
    small["unet_config"] = dict(small["unet_config"], params=dict(small["unet_config"]["params"], model_channels=32,
                                                                   channel_mult=[1], attention_resolutions=[1]))
    for bad in (dict(conditioning_key="hybrid"), dict(cond_stage_trainable=False), dict(concat_mode=True)):
        with pytest.raises(AssertionError):
            LatentDiffusionTune(**dict(small, **bad))


def test_eight_step_eta1_coefficient_rows(tune_model):
    """The rows the fine-tune walk uses against a_t, a_prev and sigma computed in float64 from the reference's own
    alphas_cumprod (g1) at the reference sampler's timesteps (g18): make_ddim_sampling_parameters, util.py:63-74."""
    model, _ = tune_model
    ac = golden("g1_schedules.npz")["alphas_cumprod"].astype(np.float64)
    ts_ref = golden("g18_tune.npz")["timesteps"]
    ts, table = model.tune_table()
    assert list(ts) == list(ts_ref) == [1 + 125 * i for i in range(8)]
    a_t = ac[ts_ref]
    a_prev = np.concatenate([ac[:1], ac[ts_ref[:-1]]])
    sigma = np.sqrt((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev))                # eta = 1
    assert table.shape == (8, 4) and table.dtype == np.float32
    for col, want in enumerate((a_t, a_prev, sigma, np.sqrt(1 - a_t))):
        np.testing.assert_allclose(table[:, col].astype(np.float64), want, rtol=5e-7, atol=0)     # a few float32 roundings
    assert (table[:, 2] > 0).all()
    # the two coefficients of the update that is linear in x and eps, as DifferentiableDDIM forms them from a row
    cx = np.sqrt(a_prev / a_t)
    ce = np.sqrt(1 - a_prev - sigma ** 2) - cx * np.sqrt(1 - a_t)
    t64 = table.astype(np.float64)
    got_cx = np.sqrt(t64[:, 1] / t64[:, 0])
    got_ce = np.sqrt(1 - t64[:, 1] - t64[:, 2] ** 2) - got_cx * t64[:, 3]
    np.testing.assert_allclose(got_cx, cx, rtol=1e-6)
    np.testing.assert_allclose(got_ce, ce, rtol=0, atol=1e-6 * np.abs(cx).max())


def test_adopt_weight_switches_at_the_threshold():
    from dsml_thesis_amd.latent_tune import adopt_weight
    assert adopt_weight(1.0, 29999, threshold=30000) == 0.0
    assert adopt_weight(1.0, 30000, threshold=30000) == 1.0
    assert adopt_weight(0.5, 0, threshold=0) == 0.5                             # the shipped YAML: on from the first step
    assert adopt_weight(2.0, 5, threshold=10, value=0.25) == 0.25


def test_fixture_was_generated_with_per_sample_timesteps():
    g = golden("g18_tune.npz")
    assert g["t"].shape == (2,) and g["t"][0] != g["t"][1]
    assert g["ddim_noise"].shape == (8, 2, 3, 16, 16) and g["image"].dtype == np.float16
    assert torch.from_numpy(g["dc12"]).shape == (2, 1, 1024)
