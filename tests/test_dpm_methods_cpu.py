"""CPU: the DPM_Solver fixtures (tests/golden/g27_dpm_methods*.npz, made by tools/make_golden_dpm_methods.py from the real reference)
checked without a GPU: the host table of `dsml_thesis_amd.dpm_solver.method_table` against the scalars the reference formed, the
singlestep order lists, the refusals and the reference's errors, the argument checks of the new entry points, one singlestep
order-3 run reproduced over the oracle's functional UNet, and the fp32 restatement of the thresholding quantile (which
tests/test_dpm_methods_ops_gpu.py holds the kernel to) against torch.quantile.

# Table tolerance: that of tests/test_dpm_cpu.py.  The table is formed with the reference's torch operations in the reference's
# order, so on one machine it has the reference's bits; 4 * 2^-23 relative allows for exp / expm1 / log of another libm build.  The
# model times, the outer time steps and r1 / r2 are held to equality.
# Run bound: max(1.5e-4, 4 d), absolute and relative, d = max |fp32 reference - float64 reference| over ALL of the run's latents."""
import types

import numpy as np
import pytest
import torch

from conftest import rnd
from dpm_methods_cases import ORDERS, RUNS, abs_quantile_rows_ref, bound, load_goldens, table_kw
from oracle import ldm_oracle as O
from oracle import weights as W

REL = 4 * 2.0 ** -23
# the columns a row of each kind carries (0, 1: alpha and sigma of the evaluation, recorded in the x0 form only)
USED = {0: (3, 4), 1: (3, 4, 5), 2: (3, 4, 5), 3: (3, 4, 5, 6, 7, 8, 9, 10, 11), 4: (3, 4), 5: (3, 4, 5, 9), 6: (3, 4, 5, 6, 7, 8, 9, 10),
        7: ()}


@pytest.fixture(scope="module")
def sched():
    return O.register_schedule(**W.SCHEDULE)


@pytest.fixture(scope="module")
def g():
    return load_goldens()


@pytest.mark.parametrize("tag", list(RUNS))
def test_host_table_against_the_reference_scalars(sched, g, tag):
    from dsml_thesis_amd.dpm_solver import STAGE_ROW, method_table
    tab = method_table(sched["alphas_cumprod"], **table_kw(tag, g))
    ref, t_in = g[tag + "_coef"], g[tag + "_t_input"]
    n = ref.shape[0]
    assert tab.orders == ORDERS[tag] == list(g[tag + "_orders"])
    assert tab.table.shape == (n, STAGE_ROW) and tab.table.dtype == torch.float32
    assert n == RUNS[tag][1]["steps"] + (1 if RUNS[tag][1].get("denoise_to_zero") else 0), "one row per model evaluation"
    assert np.array_equal(tab.t_input.numpy(), t_in), (tab.t_input.numpy(), t_in)
    assert np.array_equal(tab.table[:-1, 15].numpy(), t_in[1:]), "a row carries the model time of the next evaluation"
    assert np.array_equal(tab.timesteps.numpy(), g[tag + "_timesteps"])
    if RUNS[tag][1].get("method", "singlestep") != "multistep":
        assert np.array_equal(np.asarray(tab.r, np.float32), g[tag + "_r"]), "r1, r2 of every outer step"
    x0 = RUNS[tag][0].get("predict_x0", False)
    worst = 0.0
    for k in range(n):
        kind = int(ref[k, 2])
        assert tab.kinds[k] == kind == int(tab.table[k, 2])
        assert int(tab.table[k, 14]) & 1 == int(x0 or kind == 7)
        assert bool(int(tab.table[k, 14]) & 2) == bool(RUNS[tag][0].get("thresholding", False) and (x0 or kind == 7))
        for col in USED[kind] + ((0, 1) if (x0 or kind == 7) else ()):
            a, b = float(tab.table[k, col]), float(ref[k, col])
            worst = max(worst, abs(a - b) / abs(b))
            assert abs(a - b) <= REL * abs(b), (tag, k, col, a, b)
    print(f"{tag}: kinds {tab.kinds}, worst relative difference of a coefficient {worst:.2e} (allowed {REL:.2e})")


# get_orders_and_timesteps_for_singlestep_solver (dpm_solver.py:471-490), written out
SINGLESTEP_ORDERS = {
    1: {s: [1] * s for s in range(1, 11)},
    2: {1: [1], 2: [2], 3: [2, 1], 4: [2, 2], 5: [2, 2, 1], 6: [2, 2, 2], 7: [2, 2, 2, 1], 8: [2, 2, 2, 2], 9: [2, 2, 2, 2, 1],
        10: [2, 2, 2, 2, 2]},
    3: {1: [1], 2: [2], 3: [2, 1], 4: [3, 1], 5: [3, 2], 6: [3, 2, 1], 7: [3, 3, 1], 8: [3, 3, 2], 9: [3, 3, 2, 1], 10: [3, 3, 3, 1]},
}
SINGLESTEP_K = {1: {s: 1 for s in range(1, 11)}, 2: {s: s // 2 + s % 2 for s in range(1, 11)}, 3: {s: s // 3 + 1 for s in range(1, 11)}}


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("steps", range(1, 11))
def test_singlestep_orders(sched, steps, order):
    from dsml_thesis_amd.dpm_solver import method_table, singlestep_orders
    want = SINGLESTEP_ORDERS[order][steps]
    assert sum(want) == steps, "the orders use up all the model evaluations"
    assert singlestep_orders(steps, order) == (want, SINGLESTEP_K[order][steps])
    tab = method_table(sched["alphas_cumprod"], steps=steps, order=order)
    assert tab.orders == want and tab.table.shape[0] == steps and tab.timesteps.shape[0] == len(want) + 1
    stage = [j for o in want for j in range(o)]
    assert [int(k != 0) for k in tab.kinds] == [int(j != 0) for j in stage], "stage 0 rows are kind 0"
    if order > 1 or steps == 1:                            # (order 1 under logSNR: the reference's K = 1 grid, refused below)
        assert method_table(sched["alphas_cumprod"], steps=steps, order=order, skip_type="logSNR").timesteps.shape[0] == SINGLESTEP_K[order][steps] + 1
    assert method_table(sched["alphas_cumprod"], steps=steps, order=order, method="singlestep_fixed", denoise_to_zero=True).orders == [order] * (steps // order)


def _solver(**kw):
    from dsml_thesis_amd.dpm_solver import DPMSolverSampler
    model = types.SimpleNamespace(num_timesteps=1000, device=torch.device("cpu"),
                                  alphas_cumprod=O.register_schedule(**W.SCHEDULE)["alphas_cumprod"])
    return DPMSolverSampler(model).solver(**kw)            # the refusals come before the model is touched


def test_defaults_are_the_reference_constructor_s_and_sample_s():
    import inspect
    from dsml_thesis_amd.dpm_solver import DPM_Solver
    s = _solver()
    assert (s.predict_x0, s.thresholding, s.max_val) == (False, False, 1.)
    p = inspect.signature(DPM_Solver.sample).parameters
    want = dict(steps=20, t_start=None, t_end=None, order=3, skip_type="time_uniform", method="singlestep", lower_order_final=True,
                denoise_to_zero=False, solver_type="dpm_solver", atol=0.0078, rtol=0.05, intermediates=False)
    assert list(p)[1:] == ["x"] + list(want) and all(p[k].default == v for k, v in want.items())


def test_what_is_not_built_is_refused_by_name():
    from dsml_thesis_amd.dpm_solver import NoiseScheduleVP
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="adaptive"):
        _solver().sample(x, method="adaptive")
    for schedule in ("linear", "cosine"):
        with pytest.raises(NotImplementedError, match=schedule):
            NoiseScheduleVP(schedule)
    ac = O.register_schedule(**W.SCHEDULE)["alphas_cumprod"]
    ns = NoiseScheduleVP("discrete", alphas_cumprod=ac)
    assert ns.total_N == 1000 and ns.T == 1.
    betas = torch.as_tensor(O.register_schedule(**W.SCHEDULE)["betas"])
    torch.testing.assert_close(NoiseScheduleVP("discrete", betas=betas).log_alphas, ns.log_alphas, rtol=1e-5, atol=1e-6)


def test_the_reference_s_errors():
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(ValueError, match="skip_type"):
        _solver().sample(x, skip_type="karras")
    with pytest.raises(ValueError, match="order"):
        _solver().sample(x, order=4)
    with pytest.raises(ValueError, match="order"):
        _solver().sample(x, order=0, method="multistep")
    with pytest.raises(ValueError, match="'solver_type' must be either 'dpm_solver' or 'taylor'"):
        _solver().sample(x, solver_type="heun")
    with pytest.raises(ValueError, match="method"):
        _solver().sample(x, method="euler")
    with pytest.raises(AssertionError):
        _solver().sample(x, steps=2, order=3, method="multistep")            # dpm_solver.py:1078
    with pytest.raises(ValueError, match="logSNR"):
        _solver().sample(x, steps=3, order=1, skip_type="logSNR")            # K = 1 outer step for three updates: an IndexError there


def test_multistep_order_3_runs_down_where_the_reference_dies(sched):
    from dsml_thesis_amd.dpm_solver import method_table
    tab = method_table(sched["alphas_cumprod"], steps=6, order=3, method="multistep")
    assert tab.orders == [1, 2, 3, 3, 2, 1] and tab.kinds == [4, 5, 6, 6, 5, 4]


def test_sub_interval_only_changes_the_table(sched):
    from dsml_thesis_amd.dpm_solver import method_table
    tab = method_table(sched["alphas_cumprod"], steps=4, order=2, t_start=0.6, t_end=0.1, denoise_to_zero=True, predict_x0=True)
    assert tab.timesteps[0].item() == np.float32(0.6) and tab.timesteps[-1].item() == np.float32(0.1)
    assert tab.kinds == [0, 2, 0, 2, 7] and tab.t_input[-1].item() == np.float32((np.float32(0.1) - np.float32(1. / 1000)) * np.float32(1000.))


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Validation precedes any launch (the pointers are never dereferenced)."""
    from dsml_thesis_amd import lib as L
    lib = L.load()
    p = 4096
    good = dict(x=p, eps=p, table=p, step_idx=p, scale=1.0, cfg=0, x0_pre=0, s=0, keep=p, hist=p, x_prev=p, out=0, per=16, n=2, ts=p,
                n_ts=2, advance=1, n_rows=5, uses=3)

    def stage(**over):
        a = dict(good, **over)
        return lib.ldmk_dpm_stage(a["x"], a["eps"], a["table"], a["step_idx"], a["scale"], a["cfg"], a["x0_pre"], a["s"], a["keep"], a["hist"],
                                  a["x_prev"], a["out"], a["per"], a["n"], a["ts"], a["n_ts"], a["advance"], a["n_rows"], a["uses"], None)
    for name in ("x", "eps", "table", "step_idx", "x_prev"):
        assert stage(**{name: 0}) == -1 and b"null pointer" in lib.ldmk_last_error(), name
    for over in (dict(per=0), dict(per=-3), dict(n=0), dict(n=-1), dict(n_rows=0)):
        assert stage(**over) == -1 and b"must be positive" in lib.ldmk_last_error(), over
    for u in (0, 4, -1):
        assert stage(uses=u) == -1 and b"uses" in lib.ldmk_last_error(), u
    assert stage(keep=0) == -1 and b"need keep" in lib.ldmk_last_error()
    assert stage(hist=0) == -1 and b"need hist" in lib.ldmk_last_error()
    assert stage(x0_pre=p) == -1 and b"both x0_pre and s" in lib.ldmk_last_error()
    assert stage(s=p) == -1 and b"both x0_pre and s" in lib.ldmk_last_error()
    assert stage(ts=0) == -1 and b"needs ts" in lib.ldmk_last_error()
    assert stage(n_ts=0) == -1 and b"needs ts" in lib.ldmk_last_error()
    for args in ((0, p, p, p, 1.0, 0, p, 16, 2, 5), (p, 0, p, p, 1.0, 0, p, 16, 2, 5), (p, p, 0, p, 1.0, 0, p, 16, 2, 5),
                 (p, p, p, 0, 1.0, 0, p, 16, 2, 5), (p, p, p, p, 1.0, 0, 0, 16, 2, 5)):
        assert lib.ldmk_dpm_predict_x0(*args, None) == -1 and b"null pointer" in lib.ldmk_last_error(), args
    for args in ((p, p, p, p, 1.0, 0, p, 0, 2, 5), (p, p, p, p, 1.0, 0, p, 16, 0, 5), (p, p, p, p, 1.0, 0, p, 16, 2, 0)):
        assert lib.ldmk_dpm_predict_x0(*args, None) == -1 and b"must be positive" in lib.ldmk_last_error(), args
    q = lib.ldmk_abs_quantile_rows
    assert q(0, 2, 16, 0.995, 1.0, p, None) == -1 and b"null pointer" in lib.ldmk_last_error()
    assert q(p, 2, 16, 0.995, 1.0, 0, None) == -1 and b"null pointer" in lib.ldmk_last_error()
    for rows, per in ((0, 16), (-1, 16), (2, 0), (2, -5)):
        assert q(p, rows, per, 0.995, 1.0, p, None) == -1 and b"must be positive" in lib.ldmk_last_error(), (rows, per)
    assert q(p, 2, (1 << 20) + 1, 0.995, 1.0, p, None) == -1 and b"at most 2^20" in lib.ldmk_last_error()
    for bad_q in (-0.1, 1.5):
        assert q(p, 2, 16, bad_q, 1.0, p, None) == -1 and b"outside [0, 1]" in lib.ldmk_last_error()
    with pytest.raises(L.LdmkError, match="at most 2"):
        L.call("ldmk_abs_quantile_rows", p, 2, 1 << 21, 0.995, 1.0, p, None)


# ------------------------------------------------------------------------------------------ the quantile restatement
QUANTILE_SIZES = [1, 2, 3, 200, 201, 202, 1000, 3072, 3073, 12288, 16384, 16385]


@pytest.mark.parametrize("per", QUANTILE_SIZES)
def test_the_fp32_quantile_restatement_is_torch_quantile_bit_for_bit(per):
    rs = np.random.RandomState(900 + per)
    rows = [rs.standard_normal(per) * 50, rs.standard_normal(per),                      # normal data
            np.round(rs.standard_normal(per) * 2) / 2,                                  # ties everywhere
            np.full(per, -2.5), rs.standard_normal(per) * 1e-3]                         # all equal; all below the floor
    tied = rs.standard_normal(per)
    tied[np.argsort(np.abs(tied))[int(0.9 * per):]] = 3.25                               # heavy ties at the selected rank
    nan = rs.standard_normal(per)
    nan[per // 2] = np.nan
    v = np.stack(rows + [tied, nan]).astype(np.float32)
    for q, floor_val in ((0.995, 1.0), (0.5, 0.0), (0.0, 0.0), (1.0, 0.25), (0.37, 1e-3)):
        ref = torch.maximum(torch.quantile(torch.from_numpy(v).abs(), q, dim=1), torch.tensor(floor_val)).numpy()
        got = abs_quantile_rows_ref(v, q, floor_val)
        assert np.isnan(got[-1]) and np.isnan(ref[-1]), "a row holding a NaN gives NaN"
        assert np.array_equal(got.view(np.uint32)[:-1], ref.view(np.uint32)[:-1]), (per, q, got, ref)
    if per > 1:
        inf = v[:2].copy()
        inf[0, :] = np.inf                                  # a = b = inf: inf - inf
        inf[1, 0] = -np.inf                                 # one inf at the top rank
        got = abs_quantile_rows_ref(inf, 1.0, 1.0)
        ref = torch.maximum(torch.quantile(torch.from_numpy(inf).abs(), 1.0, dim=1), torch.tensor(1.0)).numpy()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)) or (np.isnan(got) == np.isnan(ref)).all() and np.array_equal(got[~np.isnan(got)], ref[~np.isnan(ref)])
        assert np.isnan(got[0])


# ------------------------------------------------------------------------------------------ one run over the oracle's UNet
def singlestep_loop(sd, cfg, tab, x_T, cond):
    """The loop restated in torch over the host table (guidance 1, x0 form): one model evaluation per row at the row's model time,
    m = (x - sigma e) / alpha, then the row's update over x_s, m_s, m_s1."""
    b = x_T.shape[0]
    x, xs = x_T, [x_T]
    x_s = m_s = m_s1 = None
    for k, kind in enumerate(tab.kinds):
        r = tab.table[k]
        e = O.apply_model(sd, cfg, x, tab.t_input[k].expand(b), [cond])
        m = (x - r[1] * e) / r[0]
        if kind == 0:
            x_s, m_s = x, m
            x = r[3] * x - r[4] * m
        else:
            assert kind in (1, 2)
            if kind == 1:
                m_s1 = m
            x = (r[3] * x_s - r[4] * m_s) + r[5] * (m - m_s)
        xs.append(x)
    assert m_s1 is not None
    return torch.stack(xs)


def test_oracle_loop_reproduces_the_ss3_6_fixture(sched, g):
    from dsml_thesis_amd.dpm_solver import method_table
    tol = bound(g, "ss3_6")
    sd = W.synth_state_dict(W.unet_param_shapes(W.FR_UNET), seed=0, gain=0.25)
    emb = torch.as_tensor(W.synth_tensor("embedding.weight", (8, 512)))
    c = emb[torch.tensor([1, 6])][:, None]
    with torch.no_grad():
        xs = singlestep_loop(sd, W.FR_UNET, method_table(sched["alphas_cumprod"], **table_kw("ss3_6", g)), rnd(231, 2, 3, 32, 32), c)
    ref = torch.from_numpy(g["ss3_6_x_inter"])
    assert xs.shape == ref.shape == (7, 2, 3, 32, 32)
    print(f"ss3_6 x_inter: max |oracle loop - reference| {(xs - ref).abs().max().item():.3e}; bound {tol:.3e}")
    torch.testing.assert_close(xs, ref, rtol=tol, atol=tol)
