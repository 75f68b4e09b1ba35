"""CPU: the PLMS fixtures (tests/golden/g22_plms*.npz, made by tools/make_golden_plms.py from the real reference classes) checked
without a GPU -- a PLMS loop written here over the oracle's functional UNet reproduces the recorded S = 5 runs -- and the host-side
refusals of `PLMSSampler`.

Bound per run: max(1.5e-4, 4 d), absolute and relative, d = max |fp32 reference - float64 reference| from the `*_f64` arrays
(guidance 1: d = 2.1e-5 -> 1.5e-4; guidance 3: d = 8.9e-5 -> 3.5e-4)."""
import types

import numpy as np
import pytest
import torch

from conftest import golden, rnd
from oracle import ldm_oracle as O
from oracle import weights as W


def run_bound(tag):
    g, g64 = golden("g22_plms.npz"), golden("g22_plms_f64.npz")
    d = max(np.abs(g[tag + k].astype(np.float64) - g64[tag + k + "_f64"].astype(np.float64)).max() for k in ("_x_inter", "_pred_x0"))
    return d, max(1.5e-4, 4 * d)


def plms_loop(sd, cfg, sched, S, x_T, cond, scale=1.0, uncond=None):
    """plms.py:115-236 restated: the Euler step, then Adams-Bashforth of order 2, 3, 4 over the last three outputs."""
    ts = O.make_ddim_timesteps(S, sched["betas"].shape[0])
    tab = O.make_ddim_tables(sched["alphas_cumprod"], ts, 0.0)
    b = x_T.shape[0]

    def model(x, step):
        t = torch.full((b,), int(step), dtype=torch.long)
        if uncond is None or scale == 1.0:
            return O.apply_model(sd, cfg, x, t, [cond])
        e_u, e_c = O.apply_model(sd, cfg, torch.cat([x] * 2), torch.cat([t] * 2), [torch.cat([uncond, cond])]).chunk(2)
        return O.cfg_combine(e_u, e_c, scale)

    def update(x, e, index):
        return O.ddim_update(x, e, tab["a_t"][index], tab["a_prev"][index], tab["sigma_t"][index], tab["sqrt_one_minus_at"][index])

    img, old, xs, ps = x_T, [], [x_T], [x_T]
    time_range = np.flip(ts)
    for i, step in enumerate(time_range):
        index = S - i - 1
        e_t = model(img, step)
        if len(old) == 0:
            x_pred, _ = update(img, e_t, index)
            e_prime = (e_t + model(x_pred, time_range[min(i + 1, S - 1)])) / 2
        elif len(old) == 1:
            e_prime = (3 * e_t - old[-1]) / 2
        elif len(old) == 2:
            e_prime = (23 * e_t - 16 * old[-1] + 5 * old[-2]) / 12
        else:
            e_prime = (55 * e_t - 59 * old[-1] + 37 * old[-2] - 9 * old[-3]) / 24
        img, pred_x0 = update(img, e_prime, index)
        old = (old + [e_t])[-3:]
        xs.append(img)
        ps.append(pred_x0)
    return torch.stack(xs), torch.stack(ps)


@pytest.mark.parametrize("tag,scale", [("sample_S5", 1.0), ("sample_S5_cfg", 3.0)])
def test_oracle_loop_reproduces_the_fixture(tag, scale):
    g = golden("g22_plms.npz")
    assert np.array_equal(g["ddim_timesteps_S5"], O.make_ddim_timesteps(5))
    d, bound = run_bound(tag)
    sd = W.synth_state_dict(W.unet_param_shapes(W.FR_UNET), seed=0, gain=0.25)
    emb = torch.as_tensor(W.synth_tensor("embedding.weight", (8, 512)))
    c = emb[torch.tensor([1, 6])][:, None]
    uc = torch.as_tensor(W.synth_tensor("uncond_embedding.weight", (1, 512)))[None].expand(2, 1, 512)
    with torch.no_grad():
        xs, ps = plms_loop(sd, W.FR_UNET, O.register_schedule(**W.SCHEDULE), 5, rnd(221, 2, 3, 32, 32), c, scale, uc)
    for name, mine in (("_x_inter", xs), ("_pred_x0", ps)):
        ref = torch.from_numpy(g[tag + name])
        assert mine.shape == ref.shape == (6, 2, 3, 32, 32)
        print(f"{tag}{name}: max |oracle loop - reference| {(mine - ref).abs().max().item():.3e}; d {d:.3e}, bound {bound:.3e}")
        torch.testing.assert_close(mine, ref, rtol=bound, atol=bound)


def _sampler():
    from dsml_thesis_amd.plms import PLMSSampler
    model = types.SimpleNamespace(num_timesteps=1000)          # the refusals come before the model is touched
    return PLMSSampler(model)


def test_eta_must_be_zero():
    with pytest.raises(ValueError, match="ddim_eta must be 0 for PLMS"):
        _sampler().make_schedule(ddim_num_steps=5, ddim_eta=0.5, verbose=False)


def test_use_original_steps_is_refused():
    from dsml_thesis_amd.lib import LdmkError
    s = _sampler()
    with pytest.raises(LdmkError, match="ddim_sigmas_for_original_num_steps"):
        s.plms_sampling(None, (2, 3, 32, 32), ddim_use_original_steps=True)
    with pytest.raises(LdmkError, match="ddim_sigmas_for_original_num_steps"):
        s.p_sample_plms(torch.zeros(2, 3, 4, 4), None, torch.zeros(2, dtype=torch.long), 0, use_original_steps=True)
