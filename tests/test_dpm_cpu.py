"""CPU: the DPM-Solver fixtures (tests/golden/g23_dpm*.npz, made by tools/make_golden_dpm.py from the real reference) checked without
a GPU: the host table of `dsml_thesis_amd.dpm_solver.step_table` against the scalars the reference formed, the order schedule, the
refusals, the argument checks of the two new entry points, and the S = 5 run reproduced over the oracle's functional UNet.

# Table tolerance.  The table is formed with the reference's torch operations in the reference's order, so on one machine it has the
# reference's bits; 4 * 2^-23 relative allows for exp / expm1 / log of another libm build.  The model times are held to equality.
# Run bound: max(1.5e-4, 4 d), absolute and relative, d = max |fp32 reference - float64 reference| over ALL of the run's latents, as
# tools/make_golden_dpm.py stored it (S = 5 guidance 1: d = 2.4e-4 on latents up to 388 -> 9.8e-4)."""
import types

import numpy as np
import pytest
import torch

from conftest import golden, rnd
from oracle import ldm_oracle as O
from oracle import weights as W

# tag -> (fixture file, S, keywords of step_table, the orders the issue names)
CASES = {
    "S5": ("g23_dpm.npz", 5, dict(order=2), [1, 2, 2, 2, 1]),
    "S5_cfg": ("g23_dpm.npz", 5, dict(order=2), [1, 2, 2, 2, 1]),
    # (order 3 is recorded with lower_order_final=False: with it the reference itself raises when the order drops to 2 over a
    # three-entry history, dpm_solver.py:773; the schedule 1, 2, 3, 3, 2, 1 is checked in test_order_schedule)
    "S6_o3": ("g23_dpm.npz", 6, dict(order=3, lower_order_final=False), [1, 2, 3, 3, 3, 3]),
    "S2": ("g23_dpm.npz", 2, dict(order=2), [1, 1]),
    "S15": ("g23_dpm_options.npz", 15, dict(order=2), [1] + [2] * 14),
    "S5_logSNR": ("g23_dpm_options.npz", 5, dict(order=2, skip_type="logSNR"), [1, 2, 2, 2, 1]),
    "S5_quadratic": ("g23_dpm_options.npz", 5, dict(order=2, skip_type="time_quadratic"), [1, 2, 2, 2, 1]),
    "S5_nolof": ("g23_dpm_options.npz", 5, dict(order=2, lower_order_final=False), [1, 2, 2, 2, 2]),
    "split_S5": ("g23_dpm_options.npz", 5, dict(order=2), [1, 2, 2, 2, 1]),
}
REL = 4 * 2.0 ** -23
USED = {1: (0, 1, 3, 4), 2: (0, 1, 3, 4, 5), 3: (0, 1, 3, 4, 5, 6, 7, 8, 9, 10)}      # the columns a row of each order carries


@pytest.fixture(scope="module")
def sched():
    return O.register_schedule(**W.SCHEDULE)


@pytest.mark.parametrize("tag", list(CASES))
def test_host_table_against_the_reference_scalars(sched, tag):
    from dsml_thesis_amd.dpm_solver import step_table
    fname, S, kw, orders = CASES[tag]
    g = golden(fname)
    tab = step_table(sched["alphas_cumprod"], S, **kw)
    assert tab.orders == orders == list(g[tag + "_orders"])
    assert tab.table.shape == (S, 12) and tab.table.dtype == torch.float32
    # the model times: bit for bit (t_input of every evaluation; the table carries the time of t_{k+1} for the advance kernel)
    assert np.array_equal(tab.t_input[:S].numpy(), g[tag + "_t_input"]), (tab.t_input[:S].numpy(), g[tag + "_t_input"])
    assert np.array_equal(tab.table[:S - 1, 11].numpy(), g[tag + "_t_input"][1:])
    assert np.array_equal(tab.timesteps.numpy(), g[tag + "_timesteps"])
    worst = 0.0
    np.testing.assert_allclose(tab.lam.numpy(), g[tag + "_lam"], rtol=REL, atol=0)
    ref = g[tag + "_coef"]
    for k, o in enumerate(orders):
        assert tab.table[k, 2].item() == o == ref[k, 2]
        for col in USED[o]:
            a, b = float(tab.table[k, col]), float(ref[k, col])
            worst = max(worst, abs(a - b) / abs(b))
            assert abs(a - b) <= REL * abs(b), (tag, k, col, a, b)
    print(f"{tag}: worst relative difference of a coefficient {worst:.2e} (allowed {REL:.2e})")


def test_time_uniform_model_times_are_the_ones_the_issue_names(sched):
    from dsml_thesis_amd.dpm_solver import step_table
    t = step_table(sched["alphas_cumprod"], 5).t_input.numpy()
    np.testing.assert_allclose(t[:3], [999.0, 799.2, 599.4], rtol=1e-6)
    assert abs(t[1] - round(float(t[1]))) > 0.1, "a real-valued model time: truncating it is an error"


@pytest.mark.parametrize("steps,order,lof,want", [
    (5, 2, True, [1, 2, 2, 2, 1]), (15, 2, True, [1] + [2] * 14), (6, 3, True, [1, 2, 3, 3, 2, 1]), (2, 2, True, [1, 1]),
    (5, 2, False, [1, 2, 2, 2, 2]), (14, 3, True, [1, 2] + [3] * 10 + [2, 1]), (15, 3, True, [1, 2] + [3] * 13),
    (3, 3, True, [1, 2, 1]), (4, 1, True, [1, 1, 1, 1]), (1, 1, True, [1])])
def test_order_schedule(steps, order, lof, want):
    from dsml_thesis_amd.dpm_solver import order_schedule
    assert order_schedule(steps, order, lof) == want


def _sampler():
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    model = types.SimpleNamespace(num_timesteps=1000, device=torch.device("cpu"),
                                  alphas_cumprod=O.register_schedule(**W.SCHEDULE)["alphas_cumprod"])
    return DPMSolverSampler(model)                         # the refusals come before the model is touched


def test_fewer_steps_than_the_order_asserts():
    from dsml_thesis_amd.dpm_solver import order_schedule
    with pytest.raises(AssertionError):
        order_schedule(1, 2)
    with pytest.raises(AssertionError):
        _sampler().sample(S=2, batch_size=2, shape=[3, 32, 32], order=3)


@pytest.mark.parametrize("kw,names", [(dict(method="singlestep"), "singlestep"), (dict(method="singlestep_fixed"), "singlestep"),
                                      (dict(method="adaptive"), "adaptive"), (dict(predict_x0=False), "noise-prediction"),
                                      (dict(thresholding=True), "thresholding"), (dict(solver_type="taylor"), "taylor")])
def test_what_is_not_built_is_refused_by_name(kw, names):
    with pytest.raises(NotImplementedError, match=names):
        _sampler().sample(S=5, batch_size=2, shape=[3, 32, 32], **kw)


def test_bad_skip_type_and_order():
    with pytest.raises(ValueError, match="skip_type"):
        _sampler().sample(S=5, batch_size=2, shape=[3, 32, 32], skip_type="karras")
    with pytest.raises(ValueError, match="order must be 1 or 2 or 3"):
        _sampler().sample(S=5, batch_size=2, shape=[3, 32, 32], order=4)


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Validation precedes any launch (the pointers are never dereferenced)."""
    from dsml_thesis_amd import lib as L
    lib = L.load()
    p = 4096
    good = dict(x=p, eps=p, table=p, step_idx=p, scale=1.0, cfg=0, hist=p, x_prev=p, pred_x0=0, per=16, n=2, ts=p, n_ts=2, advance=1,
                n_steps=5, max_order=2)

    def call(**over):
        a = dict(good, **over)
        return lib.ldmk_dpm_step(a["x"], a["eps"], a["table"], a["step_idx"], a["scale"], a["cfg"], a["hist"], a["x_prev"], a["pred_x0"],
                                 a["per"], a["n"], a["ts"], a["n_ts"], a["advance"], a["n_steps"], a["max_order"], None)
    for name in ("x", "eps", "table", "step_idx", "hist", "x_prev"):
        assert call(**{name: 0}) == -1 and b"null pointer" in lib.ldmk_last_error(), name
    for over in (dict(per=0), dict(per=-3), dict(n=0), dict(n=-1), dict(n_steps=0)):
        assert call(**over) == -1 and b"must be positive" in lib.ldmk_last_error(), over
    for o in (0, 4, -1):
        assert call(max_order=o) == -1 and b"orders 1, 2 and 3" in lib.ldmk_last_error(), o
    assert call(ts=0) == -1 and b"needs ts" in lib.ldmk_last_error()
    assert call(n_ts=0) == -1 and b"needs ts" in lib.ldmk_last_error()
    with pytest.raises(L.LdmkError, match="orders 1, 2 and 3"):
        L.call("ldmk_dpm_step", p, p, p, p, 1.0, 0, p, p, 0, 16, 2, p, 2, 1, 5, 7, None)
    for args in ((0, p, p, 2, 32), (p, 0, p, 2, 32), (p, p, 0, 2, 32), (p, p, p, 0, 32), (p, p, p, 2, 1)):
        assert lib.ldmk_timestep_embedding_f32(*args, None) == -1 and b"ldmk_timestep_embedding_f32" in lib.ldmk_last_error(), args


def dpm_loop(sd, cfg, tab, x_T, cond):
    """The multistep loop restated in torch over the host table (guidance 1): one model evaluation per step at the real-valued
    model time, m0 = (x - sigma_s e) / alpha_s, the update of the row's order over the last data predictions."""
    b = x_T.shape[0]
    x, ms, xs = x_T, [], [x_T]
    t_in = tab.t_input
    for k, o in enumerate(tab.orders):
        r = tab.table[k]
        e = O.apply_model(sd, cfg, x, t_in[k].expand(b), [cond])
        m0 = (x - r[1] * e) / r[0]
        xt = r[3] * x - r[4] * m0
        if o == 2:
            xt = xt - 0.5 * r[4] * (r[5] * (m0 - ms[-1]))
        elif o == 3:
            d10, d11 = r[5] * (m0 - ms[-1]), r[6] * (ms[-1] - ms[-2])
            xt = xt + r[9] * (d10 + r[7] * (d10 - d11)) - r[10] * (r[8] * (d10 - d11))
        ms = (ms + [m0])[-2:]
        x = xt
        xs.append(x)
    return torch.stack(xs)


def test_oracle_loop_reproduces_the_S5_fixture(sched):
    from dsml_thesis_amd.dpm_solver import step_table
    g, g64 = golden("g23_dpm.npz"), golden("g23_dpm_f64.npz")
    d = float(g64["S5_d"])
    stored = float(np.abs(g["S5_x_inter"].astype(np.float64) - g64["S5_x_inter_f64"].astype(np.float64)).max())
    assert abs(stored - d) <= 1e-9, "S5 is stored whole: d recomputed from the arrays is the d the tool stored"
    bound = max(1.5e-4, 4 * d)
    sd = W.synth_state_dict(W.unet_param_shapes(W.FR_UNET), seed=0, gain=0.25)
    emb = torch.as_tensor(W.synth_tensor("embedding.weight", (8, 512)))
    c = emb[torch.tensor([1, 6])][:, None]
    with torch.no_grad():
        xs = dpm_loop(sd, W.FR_UNET, step_table(sched["alphas_cumprod"], 5), rnd(231, 2, 3, 32, 32), c)
    ref = torch.from_numpy(g["S5_x_inter"])
    assert xs.shape == ref.shape == (6, 2, 3, 32, 32)
    print(f"S5 x_inter: max |oracle loop - reference| {(xs - ref).abs().max().item():.3e}; d {d:.3e}, bound {bound:.3e}")
    torch.testing.assert_close(xs, ref, rtol=bound, atol=bound)
