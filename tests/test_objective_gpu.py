"""GPU: LatentDiffusion with the full objective (x0 / l1 / learned logvar / VLB) against the reference's own p_losses + autograd
(tests/golden/g25_objective.npz, tools/make_golden_objective.py), at the bounds test_p_losses_against_reference_fixture holds g9
to: loss 2e-5 relative, full gradients rtol 5e-4 / atol 2e-6 max, gradient norms 3e-4; the x0 ancestral loop at the bound of g5's
p_sample_loop_T3 test (1e-4 / 1e-4); validation, checkpoint round trips, and that the default configuration is left alone."""
import numpy as np
import pytest
import torch

from conftest import golden, rnd
from oracle import ldm_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

SMALL = dict(W.FR_UNET, model_channels=64, channel_mult=[1, 2], num_res_blocks=1, attention_resolutions=[2, 1])   # g9's TRAIN_UNET
CASES = dict(
    a=dict(parameterization="eps", loss_type="l1", l_simple_weight=0.8, original_elbo_weight=10., learn_logvar=True, logvar_init=-0.7),
    b=dict(parameterization="x0", loss_type="l2", original_elbo_weight=1., logvar_init=0.3))
N, HW, T_IDX, LR, WD = 3, 16, (17, 803, 17), 1e-4, 1e-2


@pytest.fixture(autouse=True)
def _autograd_on():
    with torch.enable_grad():
        yield


def _model(settings, cls=None, unet=SMALL, base=None):
    """A LatentDiffusion over the reduced UNet with recipe weights; the context tensor is handed in as it is (no trainable
    conditioner between the fixture's context and the UNet)."""
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.ddpm import LatentDiffusion
    cfg = dict(base or synth.fr_config(unet=unet, vq=synth.VQ_TRAIN_SMALL))
    cfg.update(settings, cond_stage_trainable=False)
    if base is not None:
        cfg["unet_config"] = dict(cfg["unet_config"], params=dict(unet))
    m = (cls or LatentDiffusion)(**cfg)
    synth.load_recipe(m.model.diffusion_model)
    return m.cuda().train()


def _inputs():
    return (rnd(101, N, 3, HW, HW).cuda(), rnd(102, N, 3, HW, HW).cuda(), rnd(103, N, 1, 512).cuda(), torch.tensor(T_IDX).cuda())


def _reference_norm(name, stats, res):
    """L2 norm of the reference gradient(s) behind one packed buffer (as test_p_losses_against_reference_fixture maps them)."""
    sq = lambda keys: sum(stats[k][1] ** 2 for k in keys) ** 0.5
    if name == "emb_all":
        return sq([p + "emb_layers.1.weight" for p in res])
    if name == "emb_all_b":
        return sq([p + "emb_layers.1.bias" for p in res])
    if name.endswith(".qkv"):
        return sq([name[:-3] + f"attn1.to_{c}.weight" for c in "qkv"])
    if name in ("te0", "te2"):
        return stats[f"time_embed.{name[2]}.weight"][1]
    direct = {"in.wpad": "input_blocks.0.0.weight", "out.wpad": "out.2.weight", "out.bpad": "out.2.bias"}
    if name in direct:
        return stats[direct[name]][1]
    table = {"c1": "in_layers.2.weight", "c2": "out_layers.3.weight", "skip": "skip_connection.weight", "pin": "proj_in.weight",
             "pout": "proj_out.weight", "o1": "attn1.to_out.0.weight", "q2": "attn2.to_q.weight", "k2": "attn2.to_k.weight",
             "v2": "attn2.to_v.weight", "o2": "attn2.to_out.0.weight", "ff2": "ff.net.2.weight", "ff1n": "ff.net.0.proj.weight"}
    suf = name.rsplit(".", 1)[-1]
    if suf in table:
        return stats[name[:-len(suf)] + table[suf]][1]
    if suf == "w":
        base = name[:-1]
        return stats[base + ("op.weight" if base + "op.weight" in stats else "conv.weight")][1]
    return stats[name][1]


@pytest.mark.parametrize("case", ["a", "b"])
def test_p_losses_against_the_reference_objective(case):
    g = golden("g25_objective.npz")
    m = _model(CASES[case])
    x0, noise, ctx, t = _inputs()
    loss, d = m.p_losses(x0, ctx, t, noise)
    tr = m.trainer()
    ref_keys = {k[len(case) + 6:] for k in g.files if k.startswith(f"{case}_dict:") and not k.endswith("_f64")}
    assert set(d) == ref_keys, (set(d), ref_keys)
    assert list(d)[-1] == "train_loss" and ("train_loss_gamma" in d) == (case == "a")
    for k in ref_keys:
        got, ref = float(d[k]), float(g[f"{case}_dict:{k}"])
        print(f"{k}: {got:.8g}  reference {ref:.8g}  float64 reference {float(g[f'{case}_dict:{k}_f64']):.8g}")
        assert abs(got - ref) <= 2e-5 * abs(ref), (k, got, ref)
    assert abs(loss.item() - float(g[f"{case}_loss"])) <= 2e-5 * float(g[f"{case}_loss"])
    torch.testing.assert_close(tr.dctx.cpu().view(N, 1, 512), torch.from_numpy(g[f"{case}_dcontext"]), rtol=5e-4, atol=1e-7)
    direct = {"out.2.bias": tr.P.g["out.bpad"][:3]}
    for k in g.files:
        if k.startswith(f"{case}_grad:") and not k.endswith("_f64"):
            name = k[len(case) + 6:]
            got, ref = direct.get(name, tr.P.g.get(name)), torch.from_numpy(g[k])
            torch.testing.assert_close(got.cpu(), ref, rtol=5e-4, atol=2e-6 * float(ref.abs().max()))
    stats = dict(zip([str(n_) for n_ in g[f"{case}_names"]], g[f"{case}_stats"]))
    res = [p for p, mm in m.model.diffusion_model._walk() if mm.kind == "res"]
    worst = (0.0, "")
    for name, gr in tr.P.g.items():
        ref, got = _reference_norm(name, stats, res), gr.double().norm().item()
        worst = max(worst, (abs(got - ref) / (ref + 1e-30), name))
        assert abs(got - ref) <= 3e-4 * ref + 1e-12, (name, got, ref)
    print("worst gradient norm error", worst)
    if case == "a":
        ref = torch.from_numpy(g["a_dlogvar"])
        dl = m._dlogvar.cpu()
        off = torch.ones(1000, dtype=torch.bool)
        off[[17, 803]] = False
        assert bool((dl[off] == 0).all())
        print("dlogvar", dl[[17, 803]].tolist(), "reference", ref[[17, 803]].tolist())
        torch.testing.assert_close(dl, ref, rtol=5e-4, atol=2e-6 * float(ref.abs().max()))
    else:
        assert m._dlogvar is None


def test_learned_logvar_takes_the_unets_adamw_step():
    """One training step: logvar after it against the reference's torch.optim.AdamW(lr=1e-4) step (a handful of fp32 roundings
    apart: rtol 1e-6).  Entries no sample sat on have a zero gradient and only decay: init (1 - lr wd), all alike."""
    g = golden("g25_objective.npz")
    m = _model(CASES["a"])
    x0, noise, ctx, t = _inputs()
    loss, d = m.training_step_latents(x0, ctx, LR, t=t, noise=noise, weight_decay=WD)
    assert abs(loss.item() - float(g["a_loss"])) <= 2e-5 * float(g["a_loss"]) and "logvar" in d
    lv = m.logvar.data.cpu()
    torch.testing.assert_close(lv, torch.from_numpy(g["a_logvar_after"]), rtol=1e-6, atol=0)
    off = torch.ones(1000, dtype=torch.bool)
    off[[17, 803]] = False
    assert bool((lv[off] == lv[off][0]).all())
    torch.testing.assert_close(lv[off], torch.full((998,), -0.7 * (1 - LR * WD)), rtol=1e-6, atol=0)
    assert bool((lv[[17, 803]] > lv[off][0]).all())                 # dlogvar < 0 there: the step raises them by ~lr
    assert m.trainer().P.step == 1 and m._logvar_m is not None


def test_training_state_and_state_dict_round_trip_logvar_and_its_moments():
    m = _model(CASES["a"])
    x0, noise, ctx, t = _inputs()
    m.training_step_latents(x0, ctx, LR, t=t, noise=noise)
    sd, st = m.state_dict(), m.training_state()
    assert "logvar" in sd and torch.equal(sd["logvar"], m.logvar.data) and set(st["logvar"]) == {"value", "m", "v"}
    other = _model(CASES["a"])
    other.load_state_dict(sd, strict=True)
    other.load_training_state(st)
    assert torch.equal(other.logvar.data, m.logvar.data)
    assert torch.equal(other._logvar_m, m._logvar_m) and torch.equal(other._logvar_v, m._logvar_v)
    assert other.trainer().P.step == 1
    for mm in (m, other):
        mm.training_step_latents(x0, ctx, LR, t=t, noise=noise)
    assert torch.equal(other.logvar.data, m.logvar.data) and torch.equal(other.trainer().P.flat, m.trainer().P.flat)
    fixed = _model(CASES["b"])
    assert "logvar" not in fixed.state_dict() and "logvar" not in fixed.training_state()


def test_x0_ancestral_loop_against_the_reference():
    """p_sample_loop(timesteps=3) of the x0 model with the reference's draws: eager, and with use_graph=True (a given noise list
    is fed step by step either way); then the captured step with its own draws: finite, and a seeded repeat replays the same run."""
    g = golden("g25_objective.npz")
    m = _model(CASES["b"]).eval()
    _, _, ctx, _ = _inputs()
    xT = rnd(254, N, 3, HW, HW).cuda()
    nz = list(torch.from_numpy(g["b_p_sample_loop_noise"]).cuda())
    ref = torch.from_numpy(g["b_p_sample_loop_T3"])
    for use_graph in (False, True):
        out = m.p_sample_loop(ctx, (N, 3, HW, HW), x_T=xT, timesteps=3, verbose=False, noise=nz, use_graph=use_graph)
        print("use_graph", use_graph, "max error", (out.cpu() - ref).abs().max().item())
        torch.testing.assert_close(out.cpu(), ref, rtol=1e-4, atol=1e-4)
    # the same chain through p_sample, one step at a time
    img = xT
    for k, i in enumerate(reversed(range(3))):
        img = m.p_sample(img, ctx, torch.full((N,), i, device="cuda", dtype=torch.long), noise=nz[k])
    assert torch.equal(img, out)
    drawn = []
    for _ in range(2):
        torch.manual_seed(3)
        drawn.append(m.p_sample_loop(ctx, (N, 3, HW, HW), x_T=xT, timesteps=3, verbose=False, use_graph=True))
    assert torch.isfinite(drawn[0]).all() and torch.equal(drawn[0], drawn[1])


def test_validation_runs_forward_only_on_live_and_ema_weights_and_touches_nothing():
    m = _model(CASES["a"])
    x0, noise, ctx, t = _inputs()
    m.training_step_latents(x0, ctx, LR, t=t, noise=noise)           # moments exist, the shadow has moved
    tr = m.trainer()
    assert not torch.equal(m._ema_flat, tr.P.flat)
    snap = lambda: [x.clone() for x in (tr.P.flat, tr.P.grad, tr.P.m, tr.P.v, m._ema_flat, m.logvar.data, m._logvar_m, m._logvar_v)]
    before, step = snap(), tr.P.step
    calls = []
    import dsml_thesis_amd.train_ops as T
    real = T.diffusion_loss

    def spy(*a, **k):
        calls.append((k.get("want_dpred"), k.get("want_dlogvar")))
        return real(*a, **k)
    T.diffusion_loss = spy
    try:
        val = m.validation_step_latents(x0, ctx, t=t, noise=noise)
    finally:
        T.diffusion_loss = real
    assert calls == [(False, False), (False, False)], calls          # forward only, twice, no dpred
    for a, b in zip(before, snap()):
        assert torch.equal(a, b), "validation must leave the training state bit for bit"
    assert tr.P.step == step
    keys = {"val_loss_simple", "val_loss_gamma", "logvar", "val_loss_vlb", "val_loss"}
    assert set(val) == keys | {k + "_ema" for k in keys}, set(val)
    # the live entries are the training forward's; the _ema entries those of a model that holds the shadow
    _, train = m.p_losses(x0, ctx, t, noise)
    other = _model(CASES["a"])
    other.trainer().P.flat.copy_(m._ema_flat)
    other.logvar.data.copy_(m.logvar.data)
    _, shadow = other.p_losses(x0, ctx, t, noise)
    for k in keys - {"logvar"}:
        assert torch.equal(val[k], train["train" + k[3:]]), k
        assert torch.equal(val[k + "_ema"], shadow["train" + k[3:]]), k
        assert not torch.equal(val[k], val[k + "_ema"]), k
    assert torch.equal(val["logvar"], train["logvar"])
    # the default objective validates through the same kernel, with the reference's three keys
    dflt = _model({})
    val = dflt.validation_step_latents(x0, ctx, t=t, noise=noise)
    assert set(val) == {k + s for k in ("val_loss_simple", "val_loss_vlb", "val_loss") for s in ("", "_ema")}
    loss, _ = dflt.p_losses(x0, ctx, t, noise)
    assert abs(float(val["val_loss"]) - loss.item()) <= 1e-6 * loss.item()     # ldmk_mse_grad's sum, in another order


def test_batch_level_validation_and_training_steps():
    """validation_step / training_step from a batch (images -> first stage -> latents, labels -> the trainable class embedder)
    with the full objective: what `monitor: val/loss_simple_ema` reads exists, and without an EMA the '_ema' entries repeat the
    live ones as the reference's empty ema_scope makes them."""
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.ddpm import LatentDiffusion
    batch = {"image": torch.tanh(rnd(31, 2, 32, 32, 3)).cuda(), "class_label": torch.tensor([1, 5]).cuda()}
    for use_ema in (True, False):
        m = LatentDiffusion(**dict(synth.fr_config(unet=SMALL, vq=synth.VQ_TRAIN_SMALL), use_ema=use_ema, **CASES["a"]))
        for part in (m.model.diffusion_model, m.first_stage_model, m.cond_stage_model):
            synth.load_recipe(part)
        m = m.cuda().train()
        m.cond_stage_model.p_uncond = 0.0
        m.learning_rate = LR
        torch.manual_seed(0)
        loss = m.training_step(batch, 0)
        assert np.isfinite(loss.item()) and m.trainer().P.step == 1
        lv = m.logvar.data.clone()
        val = m.validation_step(batch, 0)
        assert "val_loss_simple_ema" in val and all(np.isfinite(float(v)) for v in val.values())
        assert torch.equal(m.logvar.data, lv) and m.trainer().P.step == 1
        if not use_ema:
            assert all(torch.equal(val[k], val[k + "_ema"]) for k in val if not k.endswith("_ema"))


def test_default_configuration_keeps_its_launch_and_its_two_keys(monkeypatch):
    import dsml_thesis_amd.train_ops as T
    count = dict(mse=0, full=0)
    real_mse, real_full = T.mse_grad, T.diffusion_loss
    monkeypatch.setattr(T, "mse_grad", lambda *a, **k: (count.__setitem__("mse", count["mse"] + 1), real_mse(*a, **k))[1])
    monkeypatch.setattr(T, "diffusion_loss", lambda *a, **k: (count.__setitem__("full", count["full"] + 1), real_full(*a, **k))[1])
    x0, noise, ctx, t = _inputs()
    m = _model({})
    loss, d = m.p_losses(x0, ctx, t, noise)
    assert count == dict(mse=1, full=0) and set(d) == {"train_loss_simple", "train_loss"} and np.isfinite(loss.item())
    m = _model(CASES["b"])
    m.p_losses(x0, ctx, t, noise)
    assert count == dict(mse=1, full=1)


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_two_condition_model_l1_learned_logvar_against_float64_autograd(compute):
    """LatentDiffusion2Cond (cross-attention tokens + channel-concat latents) with l1 and a learned logvar: loss and every
    gradient against float64 autograd on the oracle forward, at the bounds of the trainer-level sibling tests (f32:
    test_talking_face_unet_gradients_with_channel_concat, loss 2e-5, gradients 1e-4 of their max; bf16:
    test_bf16_training_step_gradients_against_float64_autograd, loss 5e-3, relative L2 3e-2 per tensor).
    The l1 gradient is sign(d), which jumps at d = 0.  A bf16 forward is ~1e-2 off, so it flips the sign of the ~0.6 % of the
    elements with |d| below that, each flip an error of twice the element's gradient: ~15 % of dpred in L2, which says nothing
    about the backward pass.  The bf16 bound on the gradients is a bound on the GEMMs' rounding, so the bf16 case differentiates
    sum(s d) with s = sign(d) taken from the step's own forward -- equal to |d| wherever the signs agree, and with the gradient
    s everywhere; loss, loss dictionary and dlogvar are held to the plain float64 |d| in both cases."""
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.ddpm import LatentDiffusion2Cond
    from dsml_thesis_amd.train import reference_grad_layout
    cfg = dict(SMALL, in_channels=9, context_dim=1024)
    settings = dict(loss_type="l1", learn_logvar=True, logvar_init=-0.5, l_simple_weight=0.8, original_elbo_weight=2.0)
    m = _model(settings, cls=LatentDiffusion2Cond, unet=cfg, base=synth.tf_config())
    m.train_compute = compute
    sd = W.synth_state_dict(W.unet_param_shapes(cfg))
    n = 2
    x0, noise, c34 = rnd(21, n, 3, HW, HW), rnd(12, n, 3, HW, HW), rnd(22, n, 6, HW, HW)
    c12, t = rnd(13, n, 1, 1024), torch.tensor([17, 803])
    sched = O.register_schedule(**W.SCHEDULE)
    sdg = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    a = sched["sqrt_alphas_cumprod"][t].view(-1, 1, 1, 1)
    b = sched["sqrt_one_minus_alphas_cumprod"][t].view(-1, 1, 1, 1)
    xin = torch.cat([a * x0 + b * noise, c34], 1).double()
    loss, d = m.p_losses(x0.cuda(), c12.cuda(), c34.cuda(), t.cuda(), noise.cuda())
    tr = m.trainer()
    lv = m.logvar.detach().double().cpu().requires_grad_(True)
    diff = O.unet_forward(sdg, cfg, xin, t, c12.double()) - noise.double()
    w = m.lvlb_weights.double().cpu()[t]
    objective = lambda ls: (settings["l_simple_weight"] * (ls / torch.exp(lv[t]) + lv[t]).mean() +
                            settings["original_elbo_weight"] * (w * ls).mean())
    loss_ref = objective(diff.abs().mean((1, 2, 3)))
    if compute == "f32":
        loss_ref.backward()
    else:
        s_own = torch.sign(tr.eps_pad[..., :3].permute(0, 3, 1, 2).cpu() - noise).double()
        print("signs that differ from the float64 forward's:", int((s_own != torch.sign(diff.detach())).sum()), "of", s_own.numel())
        objective((diff * s_own).mean((1, 2, 3))).backward(inputs=list(sdg.values()))
        loss_ref.backward(inputs=[lv])
    print("loss", loss.item(), "float64 autograd", loss_ref.item())
    assert set(d) == {"train_loss_simple", "train_loss_gamma", "logvar", "train_loss_vlb", "train_loss"}
    assert abs(loss.item() - loss_ref.item()) <= (2e-5 if compute == "f32" else 5e-3) * abs(loss_ref.item())
    gdev = {k: (torch.zeros_like(sd[k]) if v.grad is None else v.grad.float()).cuda() for k, v in sdg.items()}
    worst = (0.0, "")
    for name, gr in tr.P.g.items():
        ref, got = reference_grad_layout(m.model.diffusion_model, name, gdev).double().cpu(), gr.double().cpu()
        if compute == "f32":
            err = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-12)
            assert err <= 1e-4, f"gradient {name}: relative max error {err:.3e}"
        else:
            nrm = ref.norm().item()
            if nrm < 1e-12:
                assert got.abs().max().item() == 0.0, name
                continue
            err = (got - ref).norm().item() / nrm
            assert err <= 3e-2, f"bf16 gradient {name}: relative L2 error {err:.3e}"
        worst = max(worst, (err, name))
    print("worst gradient error", worst)
    dl, ref = m._dlogvar.double().cpu(), lv.grad
    print("dlogvar", dl[t].tolist(), "float64 autograd", ref[t].tolist())
    tol = 1e-4 if compute == "f32" else 3e-2
    assert bool((dl[ref == 0] == 0).all()) and (dl - ref).abs().max().item() <= tol * ref.abs().max().item()
    # validation with training_step_latents' conditioning arguments: the class embedding and the audio feature make up c12
    batch, audio = {"class_label": torch.tensor([1, 5]).cuda()}, rnd(14, n, 1, 768).cuda()
    with torch.no_grad():
        c12v = torch.cat([m.cond_stage_model_1(batch), audio], 2)
    flat, grad = tr.P.flat.clone(), tr.P.grad.clone()
    val = m.validation_step_latents(x0.cuda(), batch, audio, c34.cuda(), t=t.cuda(), noise=noise.cuda())
    assert torch.equal(tr.P.flat, flat) and torch.equal(tr.P.grad, grad)
    assert set(val) == {k + s for k in ("val_loss_simple", "val_loss_gamma", "logvar", "val_loss_vlb", "val_loss") for s in ("", "_ema")}
    _, train = m.p_losses(x0.cuda(), c12v, c34.cuda(), t.cuda(), noise.cuda())
    assert torch.equal(val["val_loss"], train["train_loss"]) and not torch.equal(val["val_loss"], val["val_loss_ema"])
