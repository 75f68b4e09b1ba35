"""GPU: EncoderUNetTrainer, NoisyLatentImageClassifier and ClassifierGuidance against the reference's own q_sample +
EncoderUNetModel + F.cross_entropy + autograd (tests/golden/g26_classifier.npz, tools/make_golden_classifier.py), compute "f32", at
the bounds test_p_losses_against_reference_fixture / test_objective_gpu.py hold g9 and g25 to: loss 2e-5 relative, full gradients
rtol 5e-4 / atol 2e-6 max, gradient norms 3e-4; logits, dx and the log-probability gradient at the full-gradient bound.  One AdamW
step at the bound of test_full_fr_unet_gradients_and_adamw_step (rtol 1e-6 / atol 1e-7: with gradients inside 5e-4 the first
Adam update lr g / (|g| + eps) moves by at most lr 5e-4 / 4 = 1.25e-8; the k third of AttentionPool2d's qkv bias, whose true
gradient is zero, at twice the reference's own fp32-to-float64 deviation).  The guided DDIM run takes S = 4: with the 1000-step
schedule S = 3 asks for timestep 1000 (ddim_timesteps = range(0, 1000, 333) + 1), in the reference as here.  bf16 compute: the bounds of
test_bf16_training_step_gradients_against_float64_autograd (loss within 5e-3, relative L2 error 3e-2), here on the logits."""
import numpy as np
import pytest
import torch

from conftest import golden, rnd
from oracle import ldm_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

SMALL16 = dict(W.FR_UNET, model_channels=64, channel_mult=[1, 2], num_res_blocks=1, attention_resolutions=[2, 1], image_size=16)
CASES = dict(adaptive=dict(pool="adaptive"), attention=dict(pool="attention"), spatial=dict(pool="spatial"),
             spatial_v2=dict(pool="spatial_v2"), attention_new=dict(pool="attention", use_new_attention_order=True))
N, HW, K, T_IDX, LABELS, LR, WD = 3, 16, 8, (17, 803, 17), (1, 7, 1), 1e-4, 1e-2


@pytest.fixture(scope="module")
def g():
    return golden("g26_classifier.npz")


@pytest.fixture(scope="module")
def inputs():
    from dsml_thesis_amd import train_ops as T
    sched = O.register_schedule(**W.SCHEDULE)
    sa, sb = sched["sqrt_alphas_cumprod"].cuda().contiguous(), sched["sqrt_one_minus_alphas_cumprod"].cuda().contiguous()
    x0, noise = rnd(261, N, 3, HW, HW).cuda(), rnd(262, N, 3, HW, HW).cuda()
    t, y = torch.tensor(T_IDX).cuda(), torch.tensor(LABELS).cuda()
    return dict(x0=x0, noise=noise, t=t, y=y, x_noisy=T.q_sample(x0, noise, t, sa, sb))


def _encoder(case):
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.encoder_unet import EncoderUNetModel
    m = EncoderUNetModel(**dict(SMALL16, in_channels=3, out_channels=K, **CASES[case]))
    synth.load_recipe(m)
    return m.cuda()


def _trainer(case, **kw):
    from dsml_thesis_amd.train import EncoderUNetTrainer
    m = _encoder(case)
    return m, EncoderUNetTrainer(m, **kw)


def _full(got, ref, what=""):
    ref = torch.as_tensor(ref)
    torch.testing.assert_close(got.detach().cpu().float(), ref, rtol=5e-4, atol=2e-6 * float(ref.abs().max()), msg=lambda m: f"{what}: {m}")


def _packed_part(t):
    return t.reshape(t.shape[0], -1).t()[:8, :128]


def _step(tr, inputs, scale=None):
    from dsml_thesis_amd import train_ops as T
    logits = tr.forward(inputs["x_noisy"], inputs["t"])
    per, mean, dl = T.cross_entropy(logits, inputs["y"], scale=scale)
    dx = tr.backward(dl)
    return logits, per, mean, dx


@pytest.mark.parametrize("case", list(CASES))
def test_step_against_the_reference(case, g, inputs):
    m, tr = _trainer(case, want_dx=True)
    logits, per, mean, dx = _step(tr, inputs)
    ref_loss = float(g[f"{case}_loss"])
    print(f"{case}: loss {mean.item():.8g}  reference {ref_loss:.8g}  float64 reference {float(g[f'{case}_loss_f64']):.8g}")
    assert abs(mean.item() - ref_loss) <= 2e-5 * abs(ref_loss)
    ref_per = torch.from_numpy(g[f"{case}_loss_per"])
    assert bool(((per.cpu() - ref_per).abs() <= 2e-5 * ref_per.abs()).all()), (per.cpu(), ref_per)
    _full(logits, g[f"{case}_logits"], "logits")
    _full(dx, g[f"{case}_dx"], "dx")
    grads = tr.state_dict_reference(tr.P.grad)
    names = [str(k) for k in g[f"{case}_names"]]
    assert list(grads) == names
    seen = 0
    for k in g.files:
        if k.endswith("_f64") or not k.startswith(case + "_grad"):
            continue
        kind, name = k[len(case) + 1:].split(":", 1)
        got = grads[name] if kind == "grad" else _packed_part(grads[name])
        _full(got, g[k], k)
        seen += 1
    assert seen >= 9
    stats = dict(zip(names, g[f"{case}_stats"]))
    worst = (0.0, "")
    for name, gr in grads.items():
        ref, got = float(stats[name][1]), gr.double().norm().item()
        worst = max(worst, (abs(got - ref) / (ref + 1e-30), name))
        assert abs(got - ref) <= 3e-4 * ref + 1e-12, (name, got, ref)
    print("worst gradient norm error", worst)
    # the guidance direction: d/dx sum_b log p(y_b | x_b, t_b), dlogits = onehot - softmax
    _, _, _, dlogp = _step(tr, inputs, scale=-1.0)
    _full(dlogp, g[f"{case}_logp_grad"], "logp_grad")


@pytest.mark.parametrize("case", ["attention", "spatial_v2"])
def test_two_identical_steps_are_bitwise_equal(case, inputs):
    m, tr = _trainer(case, want_dx=True)
    a = _step(tr, inputs)
    ga = tr.P.grad.clone()
    b = _step(tr, inputs)
    assert all(torch.equal(p, q) for p, q in zip(a, b)) and torch.equal(ga, tr.P.grad)
    assert float(ga.abs().max()) > 0


@pytest.mark.parametrize("case", list(CASES))
def test_one_adamw_step_against_the_reference(case, g, inputs):
    m, tr = _trainer(case)
    mean, per, logits = tr.classify_loss(inputs["x_noisy"], inputs["t"], inputs["y"])
    tr.adamw_step(LR, weight_decay=WD)
    after = tr.state_dict_reference()
    seen, worst = 0, 0.0
    for k in g.files:
        if k.endswith("_f64") or not k.startswith(case + "_after"):
            continue
        kind, name = k[len(case) + 1:].split(":", 1)
        got = (after[name] if kind == "after" else _packed_part(after[name])).cpu()
        ref, ref64 = torch.from_numpy(g[k]), torch.from_numpy(g[k + "_f64"])
        worst = max(worst, float((got - ref).abs().max()))
        # AttentionPool2d's k bias has an exactly zero gradient (the softmax does not see a shift of every logit): what autograd
        # leaves there is rounding noise of 1e-9, and Adam's first step turns its sign into a move of up to lr.  So the three
        # thirds [q | k | v] of qkv_proj.bias are judged apart, and a part on which the reference's own fp32 run leaves the
        # bound against its float64 twin is held to twice that deviation instead
        parts = 3 if name == "out.2.qkv_proj.bias" else 1
        for gp, rp, r64 in zip(got.reshape(parts, -1), ref.reshape(parts, -1), ref64.reshape(parts, -1)):
            dev = float((rp - r64).abs().max())
            atol = 1e-7 if bool(((rp - r64).abs() <= 1e-7 + 1e-6 * r64.abs()).all()) else 2 * dev
            if atol != 1e-7:
                print(f"{k}: the reference's fp32 is {dev:.3e} from its float64 twin; bound {atol:.3e}, ours {float((gp - rp).abs().max()):.3e}")
            torch.testing.assert_close(gp, rp, rtol=1e-6, atol=atol, msg=lambda m_: f"{k}: {m_}")
        seen += 1
    print(f"{case}: {seen} tensors after one AdamW step, worst |difference| {worst:.3e}")
    assert seen >= 9 and tr.P.step == 1
    # the columns that pad the K classes to the GEMMs' 32 stay exact zeros
    assert float(tr.P.p[tr._final + "wpad"][:, K:].abs().max()) == 0 and float(tr.P.p[tr._final + "bpad"][K:].abs().max()) == 0


@pytest.mark.parametrize("case", ["attention", "spatial"])
def test_state_dict_round_trip_gives_the_same_logits(case, inputs):
    from dsml_thesis_amd.encoder_unet import EncoderUNetModel
    m, tr = _trainer(case)
    back = tr.state_dict_reference()
    for k, v in m.state_dict().items():
        assert torch.equal(back[k], v), k                 # packed -> reference layout reproduces the loaded weights bit for bit
    tr.classify_loss(inputs["x_noisy"], inputs["t"], inputs["y"])
    tr.adamw_step(LR, weight_decay=WD)
    logits = tr.forward(inputs["x_noisy"], inputs["t"], keep_tape=False)
    fresh = EncoderUNetModel(**dict(SMALL16, in_channels=3, out_channels=K, **CASES[case])).cuda()
    fresh.load_state_dict(tr.state_dict_reference(), strict=True)
    assert torch.equal(fresh(inputs["x_noisy"], inputs["t"]), logits)
    assert torch.equal(tr.pack_reference_state(tr.state_dict_reference()), tr.P.flat)
    st = tr.optimizer_state()
    m2, tr2 = _trainer(case)
    tr2.load_optimizer_state(st)
    assert torch.equal(tr2.forward(inputs["x_noisy"], inputs["t"], keep_tape=False), logits) and tr2.P.step == 1


def test_bf16_compute_agrees_with_f32(inputs):
    m, tr = _trainer("attention")
    m16, tr16 = _trainer("attention", compute="bf16")
    mean, _, logits = tr.classify_loss(inputs["x_noisy"], inputs["t"], inputs["y"])
    mean16, _, logits16 = tr16.classify_loss(inputs["x_noisy"], inputs["t"], inputs["y"])
    rel = ((logits16 - logits).double().norm() / logits.double().norm()).item()
    print(f"bf16 logits: relative L2 error {rel:.3e}; loss {mean16.item():.7g} against {mean.item():.7g}")
    assert 0 < rel <= 3e-2 and abs(mean16.item() - mean.item()) <= 5e-3 * abs(mean.item())
    grel = ((tr16.P.grad - tr.P.grad).double().norm() / tr.P.grad.double().norm()).item()
    assert grel <= 3e-2, grel


# ------------------------------------------------------------------------------------------ the Lightning-shaped class
@pytest.fixture(scope="module")
def diffusion():
    """A small frozen LatentDiffusion over g9's UNet at 16x16 with an identity first stage: its latents are the batch's images."""
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.ddpm import LatentDiffusion
    cfg = synth.fr_config(unet=SMALL16)
    cfg.update(first_stage_config=dict(target="ldm.models.autoencoder.IdentityFirstStage", params=dict()), cond_stage_trainable=False)
    m = LatentDiffusion(**cfg)
    synth.load_recipe(m.model.diffusion_model, gain=0.25)
    synth.load_recipe(m.cond_stage_model)
    return m.cuda().eval()


def _classifier(diffusion, pool="attention", **kw):
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.classifier import NoisyLatentImageClassifier
    c = NoisyLatentImageClassifier(num_classes=K, pool=pool, diffusion_model=diffusion, **kw)
    synth.load_recipe(c.model)
    return c.cuda()


def test_classifier_steps_on_an_injected_diffusion_model(diffusion, g, inputs, monkeypatch):
    c = _classifier(diffusion)
    assert c.label_key == "class_label" and c.model.in_channels == 3 and c.model.pool == "attention"
    batch = dict(image=inputs["x0"].permute(0, 2, 3, 1).contiguous(), class_label=inputs["y"])
    monkeypatch.setattr(torch, "randn_like", lambda x: inputs["noise"])          # get_x_noisy's draw: the fixture's noise
    c.train()
    loss, logits, x_noisy, targets = c.shared_step(batch, t=inputs["t"])
    assert torch.equal(x_noisy, inputs["x_noisy"]) and torch.equal(targets, inputs["y"])
    ref_per = torch.from_numpy(g["attention_loss_per"])
    assert bool(((c.loss_per.cpu() - ref_per).abs() <= 2e-5 * ref_per.abs()).all())
    assert abs(loss.item() - float(g["attention_loss"])) <= 2e-5 * float(g["attention_loss"])
    assert set(c.logged) == {"train/loss", "train/acc@1", "train/acc@5"}
    gnorm = c.trainer().P.grad.double().norm().item()
    ref_norm = float(np.sqrt((g["attention_stats"][:, 1] ** 2).sum()))
    assert abs(gnorm - ref_norm) <= 3e-4 * ref_norm                               # training mode: the gradients are in P.grad
    before = c.trainer().P.flat.clone()
    l2 = c.training_step(batch)                                                    # random t: finite, leaves the weights alone
    assert bool(torch.isfinite(l2)) and torch.equal(before, c.trainer().P.flat)
    c.learning_rate = LR
    c.train_batch(batch)
    assert c.trainer().P.step == 1 and c.global_step == 1 and not torch.equal(before, c.trainer().P.flat)
    assert torch.equal(c.state_dict()["model.out.2.c_proj.bias"], c.trainer().P.p["out.2.c_proj.bpad"][:K]) and not c._dirty
    c.eval()
    c.on_validation_start()
    v = c.validation_step(batch)
    assert bool(torch.isfinite(v)) and "val/loss" in c.logged
    assert list(c.noisy_acc) == [0, 200, 400, 600, 800]
    assert all(len(a["acc@1"]) == 1 and len(a["acc@5"]) == 1 and 0.0 <= a["acc@1"][0] <= a["acc@5"][0] <= 1.0 for a in c.noisy_acc.values())
    assert c.trainer().tape == []                                                  # validation keeps no tape
    assert c(inputs["x_noisy"], inputs["t"]).shape == (N, K)


def test_guidance_equals_the_formula_and_steers_ddim(diffusion, g, inputs):
    from dsml_thesis_amd.classifier import ClassifierGuidance
    from dsml_thesis_amd.ddim import DDIMSampler
    c = _classifier(diffusion)
    grad = c.log_prob_grad(inputs["x_noisy"], inputs["t"], inputs["y"])
    _full(grad, g["attention_logp_grad"], "log_prob_grad")
    assert c._tr is None                                                           # guidance runs on a trainer of its own
    e_t = rnd(263, N, 3, HW, HW).cuda()
    cg = ClassifierGuidance(c, scale=3.0)
    out = cg.modify_score(diffusion, e_t, inputs["x_noisy"], inputs["t"], None, y=inputs["y"])
    sig = diffusion.sqrt_one_minus_alphas_cumprod[inputs["t"]].view(N, 1, 1, 1)
    want = e_t - sig * 3.0 * torch.from_numpy(g["attention_logp_grad"]).cuda()
    torch.testing.assert_close(out, want, rtol=5e-4, atol=2e-6 * float(want.abs().max()))
    assert torch.equal(out, e_t - sig * 3.0 * grad)
    # a training step in flight is not disturbed by a guidance pass
    c.train()
    c.step_latents(inputs["x0"], inputs["y"], inputs["t"], noise=inputs["noise"])
    held = c.trainer().P.grad.clone()
    c.log_prob_grad(inputs["x_noisy"], inputs["t"], inputs["y"])
    assert torch.equal(held, c.trainer().P.grad)
    c.eval()
    lab = torch.tensor([1, 6], device="cuda")[:, None]
    cond = diffusion.cond_stage_model.embedding(lab)
    kw = dict(S=4, batch_size=2, shape=[3, HW, HW], conditioning=cond, eta=0.0, x_T=rnd(264, 2, 3, HW, HW).cuda(), verbose=False)
    plain, _ = DDIMSampler(diffusion).sample(**kw)
    guided, _ = DDIMSampler(diffusion).sample(score_corrector=ClassifierGuidance(c, scale=50.0),
                                              corrector_kwargs=dict(y=torch.tensor([1, 6], device="cuda")), **kw)
    assert bool(torch.isfinite(guided).all()) and not torch.equal(plain, guided)
    with pytest.raises(ValueError, match="corrector_kwargs"):
        DDIMSampler(diffusion).sample(score_corrector=ClassifierGuidance(c, scale=1.0), **kw)
    # the same corrector under the PLMS sampler and the ancestral step
    from dsml_thesis_amd.plms import PLMSSampler
    guide = dict(score_corrector=ClassifierGuidance(c, scale=50.0), corrector_kwargs=dict(y=torch.tensor([1, 6], device="cuda")))
    p_plain, _ = PLMSSampler(diffusion).sample(**kw)
    p_guided, _ = PLMSSampler(diffusion).sample(**guide, **kw)
    assert bool(torch.isfinite(p_guided).all()) and not torch.equal(p_plain, p_guided)
    x, tt, nz = kw["x_T"], torch.tensor([500, 20], device="cuda"), rnd(265, 2, 3, HW, HW).cuda()
    a_plain = diffusion.p_sample(x, cond, tt, noise=nz)
    a_guided = diffusion.p_sample(x, cond, tt, noise=nz, **guide)
    sig = diffusion.sqrt_one_minus_alphas_cumprod[tt].view(2, 1, 1, 1)
    shift = -(diffusion.posterior_mean_coef1 * diffusion.sqrt_recipm1_alphas_cumprod)[tt].view(2, 1, 1, 1) * \
        (-sig * 50.0 * c.log_prob_grad(x, tt, guide["corrector_kwargs"]["y"]))
    # (the two results come from two fp32 evaluations of the update -- the fused kernel and the elementwise form: 8 ulp of the result)
    torch.testing.assert_close(a_guided - a_plain, shift, rtol=5e-4, atol=8 * 2.0 ** -23 * float(a_plain.abs().max()))
    assert float(shift.abs().max()) > 100 * 8 * 2.0 ** -23 * float(a_plain.abs().max())
