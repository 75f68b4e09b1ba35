"""GPU: the other arm of every A/B switch the PACKAGE reads, at model level: the UNet of the reference's fixture
(g4_unet_fr.npz: inputs rnd(41, 2, 3, 32, 32), ..., tolerance 3e-5 -- tests/test_unet_gpu.py, tests/test_ps_conv_gpu.py) built
under the arm.  Every test asserts (a) that the launch program differs from the default arm's in the way the switch's table line
says -- two identical programs fail, so no arm passes vacuously --, (b) eps within 3e-5 of the fixture, and (c) torch.equal with
the default arm's eps where the contract (dsml_thesis_amd/switches.py) is "bits".  Where a route engages only above a threshold
the 32 x 32 fixture does not reach, the threshold is lowered in BOTH arms through its switch's module attribute -- which is what
exercises the threshold switches.  tests/test_switch_arms_cpu.py keeps ARMS complete."""
import pytest
import torch

from conftest import golden, rnd
from oracle import weights as W
from test_unet_gpu import close, make_unet

pytestmark = pytest.mark.gpu

# switch -> the tests that run its other arm (in this module, or the existing test that already does)
ARMS = {
    "LDMK_SPLIT_BF16": ["test_unet_gpu::test_unet_split_arithmetic_routes_against_the_reference_fixtures"],
    "LDMK_F16X2": ["test_unet_gpu::test_f16x2_heavy_tailed_weights_below_the_range_threshold"],
    "LDMK_FOLD_POUT": ["test_fold_pout_gpu::test_folded_program_against_the_unfolded_program"],
    "LDMK_ATTN_QT": ["test_ops_gpu::test_attn_self"],
    "LDMK_LN_UNFOLDED": ["test_switch_arms_model_gpu::test_unfolded_layernorm"],
    "LDMK_H2_CONV_RULE": ["test_switch_arms_model_gpu::test_long_k_convolutions_without_the_f16x2_rule"],
    "LDMK_PS": ["test_switch_arms_model_gpu::test_no_pre_split_tiles"],
    "LDMK_PSC": ["test_switch_arms_model_gpu::test_no_conv_mode_pre_split_tile"],
    "LDMK_POUT_PS": ["test_switch_arms_model_gpu::test_proj_out_on_a_pre_split_tile"],
    "LDMK_ATTN_PS": ["test_switch_arms_model_gpu::test_attention_result_not_in_the_ps_layout"],
    "LDMK_ATTN_PRESPLIT": ["test_switch_arms_model_gpu::test_attention_without_the_kv_pre_pass"],
    "LDMK_QKV_TILES": ["test_switch_arms_model_gpu::test_qkv_projection_without_the_attention_tiles"],
    "LDMK_NO_WINOGRAD": ["test_switch_arms_model_gpu::test_no_winograd"],
    "LDMK_NO_SMALL_ROUTE": ["test_switch_arms_model_gpu::test_no_small_route"],
    "LDMK_SPLITK_IN_LAUNCH": ["test_switch_arms_model_gpu::test_split_k_combined_in_the_launch"],
    "LDMK_TRAIN_NO_PACKED_W": ["test_switch_arms_model_gpu::test_training_step_without_packed_bf16_weights"],
}

TOL = 3e-5
H2_ATTN = ("ldmk_attn_self_h2", "ldmk_attn_self_h2_ps", "ldmk_attn_self_h2_tiles")
WINO = ("ldmk_winograd_input", "ldmk_winograd_input_ps", "ldmk_winograd_input_ps_h2", "ldmk_upconv_gather", "ldmk_upconv_gather_ps",
        "ldmk_upconv_gather_ps_h2")


@pytest.fixture(autouse=True)
def _plan_tables_follow_the_environment():
    """set up before `monkeypatch`, hence torn down after it: the plan tables loaded under an arm do not outlive the test"""
    from dsml_thesis_amd import engine
    yield
    engine.reset_tables()


class Run:
    """one UNet forward on the fixture's inputs: eps, the launch names, the GEMM argument records, the program"""

    def __init__(self, policy=16):
        from dsml_thesis_amd import engine
        engine.reset_tables()
        m, _ = make_unet(W.FR_UNET)
        m.policy_batch = policy
        x, t, ctx = rnd(41, 2, 3, 32, 32), torch.tensor([3, 981]), rnd(42, 2, 1, 512)
        self.eps = m(x.cuda(), t.cuda(), context=ctx.cuda())
        self.pg = m.program(2, 32, 32, 1, 0)
        self.names = [c[3] for c in self.pg.calls]
        self.gemms = [c[2] for c in self.pg.calls if c[3] == "ldmk_igemm"]
        # what a launch program IS for these tests: the entry points in order, and each GEMM's plan and operand layout
        self.sig = [(c[3],) + ((c[2].tile_cfg, c[2].splitk, c[2].compute, bool(c[2].a_ps), bool(c[2].out_ps), bool(c[2].attn_kv_out),
                               bool(c[2].splitk_counters)) if c[3] == "ldmk_igemm" else ()) for c in self.pg.calls]
        torch.cuda.synchronize()

    def count(self, *names):
        return sum(self.names.count(k) for k in names)

    def ps_attention_results(self):
        """attention launches that write their result in the PS layout (argument 3 of the _ps / _tiles entry points)"""
        return sum(1 for c in self.pg.calls if c[3] in ("ldmk_attn_self_h2_ps", "ldmk_attn_self_h2_tiles", "ldmk_attn_self_x3p_ps") and c[1][3])


@pytest.fixture(scope="module")
def fixture_eps():
    return golden("g4_unet_fr.npz")["fr_eps"]


@pytest.fixture(scope="module")
def default_run():
    """the shipped configuration at policy_batch 16: the default arm of every switch that needs no lowered threshold"""
    return Run()


def _hold(name, base, other, fixture_eps):
    """(a) another program, (b) the fixture's tolerance, (c) the bits where the contract says so"""
    from dsml_thesis_amd import switches
    contract = switches.SWITCHES[name][3]
    assert contract in ("bits", "tolerance")
    assert other.sig != base.sig, f"{name}: the arm's launch program is the default arm's"
    for r in (base, other):
        close(r.eps, fixture_eps, TOL, TOL)
    d = float((other.eps - base.eps).abs().max())
    print(f"{name} [{contract}]: max |eps(arm) - eps(default)| = {d:.3e}, vs the fixture {float((other.eps.cpu() - torch.from_numpy(fixture_eps)).abs().max()):.3e}")
    if contract == "bits":
        assert torch.equal(other.eps, base.eps), f"{name} promises the default arm's bits: max |diff| {d:.3e}"


def test_default_program_is_reproducible(default_run):
    """the premise of every comparison below: two builds of the default arm are one program and give the same bits"""
    again = Run()
    assert again.sig == default_run.sig and torch.equal(again.eps, default_run.eps)


def test_unfolded_layernorm(monkeypatch, default_run, fixture_eps):
    monkeypatch.setenv("LDMK_LN_UNFOLDED", "1")
    other = Run()
    assert default_run.count("ldmk_ln_stats_guard", "ldmk_ln_stats_ps", "ldmk_ln_stats_ps_h2") > 0
    assert other.count("ldmk_ln_stats") > 0 and other.count("ldmk_ln_stats_guard", "ldmk_ln_stats_ps", "ldmk_ln_stats_ps_h2") == 0
    _hold("LDMK_LN_UNFOLDED", default_run, other, fixture_eps)


def test_long_k_convolutions_without_the_f16x2_rule(monkeypatch, fixture_eps):
    """LDMK_H2_CONV_RULE is read at import (engine.H2_CONV_MIN_K).  The rule is for direct 3x3 convolutions nobody tabled: with
    Winograd and the conv-mode tile off in both arms the low-resolution convolutions are such."""
    from dsml_thesis_amd import engine, lib as L
    monkeypatch.setenv("LDMK_NO_WINOGRAD", "1")
    monkeypatch.setenv("LDMK_PSC", "0")
    assert engine.H2_CONV_MIN_K == 1440
    base = Run()
    monkeypatch.setattr(engine, "H2_CONV_MIN_K", 1 << 30)          # what LDMK_H2_CONV_RULE=0 sets
    other = Run()
    long_h2 = lambda r: sum(1 for a in r.gemms if a.a_mode == L.A_CONV3X3 and a.K >= 1440 and a.compute == L.COMPUTE_F16X2)
    assert long_h2(base) > long_h2(other), (long_h2(base), long_h2(other))
    _hold("LDMK_H2_CONV_RULE", base, other, fixture_eps)


def test_no_pre_split_tiles(monkeypatch, default_run, fixture_eps):
    monkeypatch.setenv("LDMK_PS", "0")
    other = Run()
    assert sum(1 for a in default_run.gemms if a.a_ps) > 0 and sum(1 for a in other.gemms if a.a_ps) == 0
    _hold("LDMK_PS", default_run, other, fixture_eps)


def test_no_conv_mode_pre_split_tile(monkeypatch, default_run, fixture_eps):
    from dsml_thesis_amd import lib as L
    monkeypatch.setenv("LDMK_PSC", "0")
    other = Run()
    conv_ps = lambda r: sum(1 for a in r.gemms if a.a_ps and a.a_mode == L.A_CONV3X3)
    assert conv_ps(default_run) > 0 and conv_ps(other) == 0 and default_run.count("ldmk_gn_apply_ps_h2") > other.count("ldmk_gn_apply_ps_h2") == 0
    _hold("LDMK_PSC", default_run, other, fixture_eps)


def test_proj_out_on_a_pre_split_tile(monkeypatch, fixture_eps):
    """proj_out is its own GEMM only where the last block's ff.net.2 did not take it along (LDMK_FOLD_POUT=0 in both arms), and it
    follows ff.net.2 onto a pre-split tile only where that GEMM does not split K: at the fixture's size the plans of a 64-sample job
    (policy_batch 64: 65536 and 16384 rows at the 160- and 320-channel levels), not those of 16 samples, which all split K."""
    monkeypatch.setenv("LDMK_FOLD_POUT", "0")
    base = Run(policy=64)
    monkeypatch.setenv("LDMK_POUT_PS", "1")
    other = Run(policy=64)
    ps_out = lambda r: sum(1 for a in r.gemms if a.a_ps and a.out_ps)
    assert sum(1 for a in other.gemms if a.a_ps) > sum(1 for a in base.gemms if a.a_ps) and ps_out(other) > ps_out(base)
    _hold("LDMK_POUT_PS", base, other, fixture_eps)


def test_attention_result_not_in_the_ps_layout(monkeypatch, default_run, fixture_eps):
    monkeypatch.setenv("LDMK_ATTN_PS", "0")
    other = Run()
    assert default_run.ps_attention_results() > 0 and other.ps_attention_results() == 0
    _hold("LDMK_ATTN_PS", default_run, other, fixture_eps)


def test_attention_without_the_kv_pre_pass(monkeypatch, default_run, fixture_eps):
    """The bf16x3 attention splits K / V by a pre-pass from LDMK_ATTN_PRESPLIT_MIN_TOKENS (2048) tokens; the fixture's bf16x3
    attentions have fewer.  At the shipped threshold no launch of the program is pre-split; lowered to 1 (unet.ATTN_PRESPLIT_MIN_TOKENS,
    read at import) in both arms, every bf16x3 attention is -- unless LDMK_ATTN_PRESPLIT=0."""
    from dsml_thesis_amd import unet
    assert unet.ATTN_PRESPLIT_MIN_TOKENS == 2048 and default_run.count("ldmk_attn_self_x3p", "ldmk_attn_self_x3p_ps") == 0
    n_x3 = default_run.count("ldmk_attn_self_x3")
    assert n_x3 > 0
    monkeypatch.setattr(unet, "ATTN_PRESPLIT_MIN_TOKENS", 1)
    base = Run()
    assert base.count("ldmk_attn_self_x3p", "ldmk_attn_self_x3p_ps") == n_x3 and base.count("ldmk_attn_self_x3") == 0
    assert torch.equal(base.eps, default_run.eps), "the pre-pass form promises the bits of ldmk_attn_self_x3 (the threshold is a route)"
    monkeypatch.setenv("LDMK_ATTN_PRESPLIT", "0")
    other = Run()
    assert other.count("ldmk_attn_self_x3p", "ldmk_attn_self_x3p_ps") == 0 and other.count("ldmk_attn_self_x3") == n_x3
    _hold("LDMK_ATTN_PRESPLIT", base, other, fixture_eps)


def test_qkv_projection_without_the_attention_tiles(monkeypatch, default_run, fixture_eps):
    monkeypatch.setenv("LDMK_QKV_TILES", "0")
    other = Run()
    kv = lambda r: sum(1 for a in r.gemms if a.attn_kv_out)
    assert kv(default_run) > 0 and default_run.count("ldmk_attn_self_h2_tiles") == kv(default_run)
    assert kv(other) == 0 and other.count("ldmk_attn_self_h2_tiles") == 0 and other.count(*H2_ATTN) == default_run.count(*H2_ATTN)
    _hold("LDMK_QKV_TILES", default_run, other, fixture_eps)


def test_no_winograd(monkeypatch, fixture_eps):
    """The Winograd / phase-split routes at the fixture's sizes: thresholds lowered in both arms as in
    test_unet_gpu.test_unet_winograd_route_against_the_reference_fixtures (NetBuilder.WINO_MIN_TILES is LDMK_WINO_MIN_TILES read at
    import), the conv-mode tile off so that the wide convolutions take them."""
    from dsml_thesis_amd.engine import NetBuilder
    assert NetBuilder.WINO_MIN_TILES == 256 and NetBuilder.WINO_MIN_CIN == 320
    monkeypatch.setattr(NetBuilder, "WINO_MIN_TILES", 1)
    monkeypatch.setattr(NetBuilder, "UP_MIN_PIXELS", 1)
    monkeypatch.setenv("LDMK_PSC", "0")
    base = Run()
    assert base.count(*WINO) >= 12
    monkeypatch.setattr(NetBuilder, "WINO_MIN_CIN", 1 << 30)       # the threshold switch alone turns the routes off as well
    assert Run().count(*WINO) == 0
    monkeypatch.setattr(NetBuilder, "WINO_MIN_CIN", 320)
    monkeypatch.setenv("LDMK_NO_WINOGRAD", "1")
    other = Run()
    assert other.count(*WINO) == 0 and other.count("ldmk_winograd_output", "ldmk_upconv_scatter") == 0
    _hold("LDMK_NO_WINOGRAD", base, other, fixture_eps)


def test_no_small_route(monkeypatch, fixture_eps):
    """The batch-2 job as test_unet_gpu runs it for the small-batch route (policy_batch None); LDMK_SMALL_ROWS (unet_small.SMALL_ROWS,
    read at import) below the job's 2048 rows turns the route off like the switch does."""
    from dsml_thesis_amd import unet_small
    base = Run(policy=None)
    assert getattr(base.pg, "small_route", False) and "ldmk_post" in base.names and "ldmk_attn_self_small" in base.names
    assert unet_small.SMALL_ROWS == 4096
    monkeypatch.setattr(unet_small, "SMALL_ROWS", 2047)
    by_rows = Run(policy=None)
    monkeypatch.setattr(unet_small, "SMALL_ROWS", 4096)
    monkeypatch.setenv("LDMK_NO_SMALL_ROUTE", "1")
    other = Run(policy=None)
    for r in (by_rows, other):
        assert not getattr(r.pg, "small_route", False) and "ldmk_post" not in r.names and "ldmk_gn_finalize" in r.names
    assert by_rows.sig == other.sig and torch.equal(by_rows.eps, other.eps)
    _hold("LDMK_NO_SMALL_ROUTE", base, other, fixture_eps)


def test_split_k_combined_in_the_launch(monkeypatch, default_run, fixture_eps):
    monkeypatch.setenv("LDMK_SPLITK_IN_LAUNCH", "1")
    other = Run()
    inl = lambda r: sum(1 for a in r.gemms if a.splitk_counters)
    split = sum(1 for a in default_run.gemms if a.splitk > 1 and not a.a_ps and not a.raw_slabs)
    assert split > 0 and inl(default_run) == 0 and inl(other) == split
    assert [s[:4] for s in other.sig] == [s[:4] for s in default_run.sig]          # same launches, same plans: only the combine moved
    _hold("LDMK_SPLITK_IN_LAUNCH", default_run, other, fixture_eps)


def test_training_step_without_packed_bf16_weights(monkeypatch):
    """Two p_losses calls of the bf16 UNetTrainer of tests/test_bf16_gpu.py: the second reads the packed bf16 weight images the
    first registered.  With LDMK_TRAIN_NO_PACKED_W set nothing is registered and the GEMMs convert the fp32 weights themselves: the
    same loss bit for bit, on both calls."""
    from dsml_thesis_amd import switches
    from dsml_thesis_amd.train import UNetTrainer
    from oracle import ldm_oracle as O
    from test_train_gpu import SMALL, _setup
    assert switches.SWITCHES["LDMK_TRAIN_NO_PACKED_W"][3] == "bits"
    with torch.enable_grad():
        m, _, sd, x0, noise, ctx, t = _setup(SMALL, 2, 16)
        sched = O.register_schedule(**W.SCHEDULE)
        args = (x0.cuda(), ctx.cuda(), t.cuda(), noise.cuda(), sched["sqrt_alphas_cumprod"].cuda(), sched["sqrt_one_minus_alphas_cumprod"].cuda())
        tr = UNetTrainer(m, compute="bf16")
        packed = [tr.p_losses(*args).item(), tr.p_losses(*args).item()]
        assert tr._wt16.images, "the default arm packs its forward weights"
        monkeypatch.setenv("LDMK_TRAIN_NO_PACKED_W", "1")
        tr2 = UNetTrainer(m, compute="bf16")
        plain = [tr2.p_losses(*args).item(), tr2.p_losses(*args).item()]
        assert not tr2._wt16.images, "LDMK_TRAIN_NO_PACKED_W: no image may be registered"
    print(f"bf16 training loss, packed images {packed}, fp32 weights {plain}")
    assert plain[1] == packed[1] and plain == packed
