"""GPU: the training engine on the UNet variants beyond the shipped spatial-transformer one -- class-conditional ('adm':
use_scale_shift_norm + num_classes + AttentionBlock / QKVAttention), unconditional (AttentionBlock / QKVAttentionLegacy, no
context) and resblock_updown -- against PyTorch autograd run on the oracle (CPU).

The oracle casts to float32 inside its scale-shift ResBlock and its AttentionBlock (the reference's GroupNorm32), so float64
autograd raises "mixed dtype" for ADM_UNET, UPDOWN_ADM_UNET and UNCOND_UNET: those run the oracle in float32, like
test_full_fr_unet_gradients_and_adamw_step; the spatial-transformer resblock_updown UNet runs in float64.

Metric and bounds are the existing ones (tests/test_train_gpu.py): per parameter tensor max |got - ref| / max |ref| <= 1e-4,
loss within 5e-5 relative when both sides are fp32 (2e-5 against float64), context gradient 2e-4; bf16 as tests/test_bf16_gpu.py.
Every test prints the figure it asserts on (run with -s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rnd
from oracle import ldm_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _autograd_on():
    """The reference side of these tests is autograd; other test modules switch it off process-wide."""
    with torch.enable_grad():
        yield


UNCOND_SMALL = dict(W.UNCOND_UNET, image_size=16, model_channels=64, channel_mult=[1, 2], num_res_blocks=1, attention_resolutions=[2, 1])
UPDOWN_SMALL = dict(W.UPDOWN_UNET, model_channels=64, channel_mult=[1, 2], attention_resolutions=[2, 1])
LABELS = [3, 7, 3]          # a repeated label: two samples add into one row of label_emb.weight


def _setup(cfg, n, hw, compute="f32", seed=0):
    from dsml_thesis_amd.unet import UNetModel
    from dsml_thesis_amd.train import UNetTrainer
    m = UNetModel(**cfg)
    sd = W.synth_state_dict(W.unet_param_shapes(cfg))
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    tr = UNetTrainer(m, compute=compute)
    x0 = rnd(seed + 1, n, cfg["in_channels"], hw, hw)
    noise = rnd(seed + 2, n, cfg["out_channels"], hw, hw)
    ctx = rnd(seed + 3, n, 1, cfg["context_dim"]) if cfg.get("context_dim") else None
    y = torch.tensor(LABELS[:n]) if cfg.get("num_classes") else None
    t = torch.tensor([17, 803, 400, 999][:n])
    return m, tr, sd, x0, noise, ctx, y, t


def _oracle_grads(cfg, sd, x0, noise, ctx, y, t, dtype):
    sched = O.register_schedule(**W.SCHEDULE)
    sdg = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
    ctxg = None if ctx is None else ctx.to(dtype).requires_grad_(True)
    a = sched["sqrt_alphas_cumprod"][t].view(-1, 1, 1, 1)
    b = sched["sqrt_one_minus_alphas_cumprod"][t].view(-1, 1, 1, 1)
    x_noisy = (a * x0 + b * noise).to(dtype)          # q_sample in fp32 (ddpm.py:1009-1012), then promoted
    eps = O.unet_forward(sdg, cfg, x_noisy, t, ctxg, y=y)
    loss = F.mse_loss(eps, noise.to(dtype))
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in sdg.items()}, None if ctxg is None else ctxg.grad, sched


def _p_losses(tr, sched, x0, noise, ctx, y, t):
    cu = lambda v: None if v is None else v.cuda()
    return tr.p_losses(x0.cuda(), cu(ctx), t.cuda(), noise.cuda(), sched["sqrt_alphas_cumprod"].cuda(),
                       sched["sqrt_one_minus_alphas_cumprod"].cuda(), y=cu(y))


def _check(cfg, n, hw, dtype, loss_rtol):
    from test_train_gpu import _check_all_grads
    m, tr, sd, x0, noise, ctx, y, t = _setup(cfg, n, hw)
    loss_ref, grads, dctx_ref, sched = _oracle_grads(cfg, sd, x0, noise, ctx, y, t, dtype)
    for k, v in grads.items():
        assert v is not None and torch.isfinite(v).all(), k
    loss = _p_losses(tr, sched, x0, noise, ctx, y, t)
    print("loss", loss.item(), "reference", loss_ref.item(), "relative", abs(loss.item() - loss_ref.item()) / abs(loss_ref.item()))
    assert abs(loss.item() - loss_ref.item()) <= loss_rtol * abs(loss_ref.item()), (loss.item(), loss_ref.item())
    worst = _check_all_grads(m, tr, grads, 1e-4)
    print("worst gradient error", worst)
    if ctx is not None:
        err = (tr.dctx.double().cpu() - dctx_ref.view_as(tr.dctx.cpu())).abs().max().item() / dctx_ref.abs().max().item()
        print("context gradient error", err)
        assert err <= 2e-4, f"context gradient {err:.3e}"
    else:
        assert tr.dctx is None
    return m, tr, grads


# ---- 1-3: every parameter gradient of p_losses ------------------------------------------------------------------------
def test_adm_unet_gradients_film_new_order_attention_and_repeated_labels():
    """ADM_UNET (use_scale_shift_norm, 10 classes, AttentionBlock with use_new_attention_order), n = 3, 16x16, y = [3, 7, 3]:
    FiLM GroupNorm backward, the AttentionBlock tape and the label-embedding scatter with a repeated label."""
    m, tr, grads = _check(W.ADM_UNET, 3, 16, torch.float32, 5e-5)
    g = tr.P.g["label_emb.weight"].cpu()
    ref = grads["label_emb.weight"]
    used = sorted(set(LABELS))
    for k in range(W.ADM_UNET["num_classes"]):
        if k in used:
            assert g[k].abs().max().item() > 0 and ref[k].abs().max().item() > 0, k
        else:
            assert g[k].abs().max().item() == 0.0 and ref[k].abs().max().item() == 0.0, f"label row {k} must stay exactly zero"


def test_unconditional_small_unet_gradients_legacy_attention_order():
    """Reduced BASELINE configs[0] UNet: AttentionBlock / QKVAttentionLegacy ([head][q | k | v][d] qkv rows), no context."""
    _check(UNCOND_SMALL, 2, 16, torch.float32, 5e-5)


def test_unconditional_full_unet_gradients():
    """The real UNCOND_UNET (160 / 320 / 640 channels, attention at 1024 / 256 / 64 tokens) at 32x32, batch 1, float32 autograd."""
    _check(W.UNCOND_UNET, 1, 32, torch.float32, 5e-5)


def test_updown_adm_unet_gradients():
    """resblock_updown with scale-shift norm and labels: ResBlock(down=True) / ResBlock(up=True) around FiLM blocks."""
    _check(W.UPDOWN_ADM_UNET, 3, 16, torch.float32, 5e-5)


def test_updown_spatial_transformer_unet_gradients_float64():
    """resblock_updown under spatial transformers, against float64 autograd; context gradient at the existing 2e-4."""
    _check(UPDOWN_SMALL, 2, 16, torch.float64, 2e-5)


def test_odd_grid_is_refused_for_resblock_updown():
    from dsml_thesis_amd import lib as L
    m, tr, sd, x0, noise, ctx, y, t = _setup(UPDOWN_SMALL, 2, 16)
    with pytest.raises(L.LdmkError, match="odd grid"):
        tr.forward(rnd(1, 2, 3, 14, 17).cuda(), t.cuda(), ctx.cuda())


# ---- 4: training forward == sampling forward ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adm", "uncond", "updown", "updown_adm"])
def test_training_forward_matches_sampling_forward(name):
    cfg = dict(adm=W.ADM_UNET, uncond=UNCOND_SMALL, updown=UPDOWN_SMALL, updown_adm=W.UPDOWN_ADM_UNET)[name]
    n = 3 if cfg.get("num_classes") else 2
    m, tr, sd, x0, noise, ctx, y, t = _setup(cfg, n, 16)
    cu = lambda v: None if v is None else v.cuda()
    eps_t = tr.forward(x0.cuda(), t.cuda(), cu(ctx), y=cu(y))
    eps_s = m(x0.cuda(), t.cuda(), context=cu(ctx), y=cu(y))
    torch.testing.assert_close(eps_t, eps_s, rtol=2e-4, atol=2e-5)


def test_forward_argument_checks():
    from dsml_thesis_amd import lib as L
    m, tr, sd, x0, noise, ctx, y, t = _setup(W.ADM_UNET, 3, 16)
    with pytest.raises(AssertionError, match="class-conditional"):
        tr.forward(x0.cuda(), t.cuda())
    with pytest.raises(L.LdmkError, match="context must be None"):
        tr.forward(x0.cuda(), t.cuda(), rnd(5, 3, 1, 512).cuda(), y=y.cuda())
    m, tr, sd, x0, noise, ctx, y, t = _setup(UPDOWN_SMALL, 2, 16)
    with pytest.raises(L.LdmkError, match="context is required"):
        tr.forward(x0.cuda(), t.cuda())


# ---- 5: the three new kernels on their own ------------------------------------------------------------------------------
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("C", [64, 320])
@pytest.mark.parametrize("hw", [64, 1024])
def test_film_groupnorm_backward_kernel(hw, C, acc):
    """ldmk_gn_film_bwd against float64 autograd of h = SiLU((xhat gamma + beta) (1 + scale) + shift) written out here.
    Same metric and bound as the network tests (max error over max reference <= 1e-4)."""
    from dsml_thesis_amd import lib as L
    from dsml_thesis_amd import ops
    from dsml_thesis_amd import train_ops as T
    n, eps, ld, off = 2, 1e-5, 2 * C + 24, 8                   # the (scale | shift) rows sit inside wider emb_all rows
    x, dy = rnd(700, n, hw, C) * 1.5 + 0.3, rnd(701, n, hw, C)
    gamma, beta = 1 + 0.1 * rnd(702, C), 0.1 * rnd(703, C)
    film = torch.zeros(n, ld)
    film[:, off:off + 2 * C] = 0.3 * rnd(704, n, 2 * C)
    # reference
    xd, gd, bd, fd = (v.double().requires_grad_(True) for v in (x, gamma, beta, film))
    u = F.group_norm(xd.permute(0, 2, 1), 32, gd, bd, eps).permute(0, 2, 1)
    sc, sh = fd[:, None, off:off + C], fd[:, None, off + C:off + 2 * C]
    (F.silu(u * (1 + sc) + sh) * dy.double()).sum().backward()
    # kernels: the forward's records and FiLM-folded coefficients, then the backward under test
    xg, dyg, gg, bg, fg = (v.cuda() for v in (x, dy, gamma, beta, film))
    part = torch.empty(n * L.load().ldmk_gn_chunks(hw) * C * 3, device="cuda")
    L.call("ldmk_gn_partial", xg.data_ptr(), C, n, hw, part.data_ptr(), ops.stream())
    coef = torch.empty(n, 2, C, device="cuda")
    L.call("ldmk_gn_finalize", part.data_ptr(), C, None, 0, n, hw, 32, eps, gg.data_ptr(), bg.data_ptr(), coef.data_ptr(), ops.stream())
    mr = T.gn_group_stats(part, C, None, 0, n, hw, 32, eps)
    fslice = fg[:, off:off + 2 * C]
    T.gn_coef_film_(coef, fslice)
    base = [rnd(705, n, hw, C).cuda(), rnd(706, C).cuda(), rnd(707, C).cuda()] if acc else [torch.zeros(n, hw, C).cuda(), torch.zeros(C).cuda(), torch.zeros(C).cuda()]
    dx, dg, db = (b.clone() for b in base)
    dfilm_all = torch.full((n, ld), 7.0, device="cuda")
    T.gn_film_bwd(xg, dyg, coef, mr, gg, bg, fslice, n, hw, dfilm_all[:, off:off + 2 * C], dx=dx, acc_dx=acc, dgamma=dg, dbeta=db,
                  acc_params=acc)
    keep = torch.ones(n, ld, dtype=torch.bool)
    keep[:, off:off + 2 * C] = False
    assert (dfilm_all.cpu()[keep] == 7.0).all(), "d(scale | shift) must stay inside its own columns"
    for name, got, b0, ref in (("dx", dx, base[0], xd.grad), ("dgamma", dg, base[1], gd.grad), ("dbeta", db, base[2], bd.grad),
                               ("dfilm", dfilm_all[:, off:off + 2 * C], None, fd.grad[:, off:off + 2 * C])):
        got = got.double().cpu() - (0 if b0 is None else b0.double().cpu())
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        print(f"film bwd hw={hw} C={C} acc={acc} {name}: {err:.3e}")
        # with the accumulate flags the stored value is base + gradient rounded to fp32: the subtraction above gives back the
        # gradient to within half an ulp of |base| + |gradient|, which for these magnitudes stays far inside the bound
        assert err <= 1e-4, f"{name}: {err:.3e}"
    dx2, dg2, db2 = (b.clone() for b in base)
    df2 = torch.empty(n, 2 * C, device="cuda")
    T.gn_film_bwd(xg, dyg, coef, mr, gg, bg, fslice, n, hw, df2, dx=dx2, acc_dx=acc, dgamma=dg2, dbeta=db2, acc_params=acc)
    assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db) and torch.equal(df2, dfilm_all[:, off:off + 2 * C])


def test_label_embedding_backward_kernel_is_deterministic_with_repeated_labels():
    from dsml_thesis_amd import train_ops as T
    n, emb, classes = 6, 256, 10
    y = torch.tensor([3, 7, 3, 3, 0, 7])
    d = rnd(710, n, emb)
    ref = torch.zeros(classes, emb)
    for i in range(n):                       # index-ordered loop: the order the kernel promises per class row
        ref[y[i]] += d[i]
    dw = torch.full((classes, emb), 5.0, device="cuda")
    T.label_emb_bwd(d.cuda(), y.cuda(), dw)
    assert torch.equal(dw.cpu(), ref)
    for k in set(range(classes)) - set(y.tolist()):
        assert dw[k].abs().max().item() == 0.0
    again = torch.empty(classes, emb, device="cuda")
    T.label_emb_bwd(d.cuda(), y.cuda(), again)
    assert torch.equal(again, dw)
    base = rnd(711, classes, emb)
    acc = base.clone().cuda()
    T.label_emb_bwd(d.cuda(), y.cuda(), acc, accumulate=True)
    want = base.clone()
    for k in set(y.tolist()):
        want[k] = base[k] + ref[k]
    assert torch.equal(acc.cpu(), want)      # absent classes unchanged, present ones old + the ordered sum


@pytest.mark.parametrize("shape", [(2, 4, 4, 64), (3, 5, 7, 320)])
def test_average_pool_backward_kernel(shape):
    from dsml_thesis_amd import train_ops as T
    dy = rnd(720, *shape)
    ref = 0.25 * dy.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert torch.equal(T.avgpool2_bwd(dy.cuda()).cpu(), ref)
    base = rnd(721, *ref.shape)
    out = base.clone().cuda()
    T.avgpool2_bwd(dy.cuda(), out=out, accumulate=True)
    assert torch.equal(out.cpu(), base + ref)
    # it is the gradient of the forward's avg_pool2d(2, 2)
    x = rnd(722, *ref.shape).double().requires_grad_(True)
    (F.avg_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1) * dy.double()).sum().backward()
    assert torch.equal(x.grad.float(), ref)


# ---- 6: reference layout <-> flat packed layout -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adm", "uncond"])
def test_state_dict_round_trip_is_exact(name):
    """Legacy-order and new-order AttentionBlock qkv (stored in the kernels' [q | k | v][head][d] order) and label_emb."""
    cfg = dict(adm=W.ADM_UNET, uncond=UNCOND_SMALL)[name]
    m, tr, sd, *_ = _setup(cfg, 2, 16)
    back = tr.state_dict_reference()
    assert set(back) == set(sd)
    for k, v in sd.items():
        assert torch.equal(back[k].cpu(), v), k
    other = W.synth_state_dict(W.unet_param_shapes(cfg), seed=5)
    flat = tr.pack_reference_state(other)
    back = tr.state_dict_reference(flat)
    for k, v in other.items():
        assert torch.equal(back[k].cpu(), v), k
    if name == "adm":
        assert "label_emb.weight" in back
    else:      # legacy order really is a permutation here: the flat copy differs from the reference's row order
        k = "input_blocks.1.1."
        raw = tr.P.p[k + "aqkv"].t().cpu()
        assert not torch.equal(raw, sd[k + "qkv.weight"].reshape(raw.shape)) and m.input_blocks[1].layers[1].new_order is False


# ---- 7: bucketed all-reduce planning ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adm", "uncond", "updown", "updown_adm"])
def test_tape_is_in_reverse_parameter_order(name):
    from dsml_thesis_amd.train import plan_buckets
    cfg = dict(adm=W.ADM_UNET, uncond=UNCOND_SMALL, updown=UPDOWN_SMALL, updown_adm=W.UPDOWN_ADM_UNET)[name]
    n = 3 if cfg.get("num_classes") else 2
    m, tr, sd, x0, noise, ctx, y, t = _setup(cfg, n, 16)
    cu = lambda v: None if v is None else v.cuda()
    tr.forward(x0.cuda(), t.cuda(), cu(ctx), y=cu(y))
    total = tr.P.grad.numel()
    buckets = plan_buckets([off for _, off in reversed(tr.tape)], total, 1 << 16)
    spans = sorted(buckets.values())
    assert spans[0][0] == 0 and spans[-1][1] == total and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    if cfg.get("num_classes"):          # label_emb.weight sits right after the time_embed parameters
        names = [s[0] for s in tr.P.specs]
        assert names[names.index("time_embed.2.bias") + 1] == "label_emb.weight"


# ---- 8: the step inside a hipGraph ------------------------------------------------------------------------------------
def test_adm_step_replays_from_a_graph_with_the_same_bits():
    m, tr, sd, x0, noise, ctx, y, t = _setup(W.ADM_UNET, 3, 16)
    sched = O.register_schedule(**W.SCHEDULE)
    sa, sb = sched["sqrt_alphas_cumprod"].cuda(), sched["sqrt_one_minus_alphas_cumprod"].cuda()
    x0, noise, y, t = x0.cuda(), noise.cuda(), y.cuda(), t.cuda()
    shadow = tr.P.flat.clone()
    loss_buf = torch.zeros(1, device="cuda")

    def step():
        loss = tr.p_losses(x0, None, t, noise, sa, sb, y=y)
        tr.adamw_step(lr=1e-6)
        tr.ema_update(shadow, 0.9999)
        loss_buf.copy_(loss)

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    saved = [v.clone() for v in (tr.P.flat, tr.P.m, tr.P.v, shadow)]
    step()                                                   # the eager step the replay has to reproduce
    loss_e, grad_e, flat_e = loss_buf.clone(), tr.P.grad.clone(), tr.P.flat.clone()
    for dst, src in zip((tr.P.flat, tr.P.m, tr.P.v, shadow), saved):
        dst.copy_(src)
    tr.P.grad.zero_()
    tr.P.step = 2              # the bias corrections are host scalars: the captured step is step 3 again
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        step()
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss_buf, loss_e) and torch.equal(tr.P.grad, grad_e) and torch.equal(tr.P.flat, flat_e)


# ---- 9: through the LatentDiffusion facade ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [None, "adm"])
def test_latent_diffusion_trains_without_a_context(key):
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.ddpm import LatentDiffusion
    if key is None:
        cfg = synth.uncond_config(UNCOND_SMALL, synth.VQ_F4_256)
        cond, n, ch = None, 2, 4
    else:
        cfg = synth.fr_config(unet=W.ADM_UNET)
        cfg.update(conditioning_key="adm", cond_stage_trainable=False)
        cond, n, ch = torch.tensor(LABELS).cuda(), 3, 3
    model = LatentDiffusion(**cfg)
    synth.load_recipe(model.model.diffusion_model, gain=0.5)
    model = model.cuda().train()
    assert model.model.conditioning_key == key
    tr = model.trainer()
    ema0 = model._ema_flat.clone()
    z, noise, t = rnd(90, n, ch, 16, 16).cuda(), rnd(93, n, ch, 16, 16).cuda(), torch.tensor([300, 800, 500][:n]).cuda()
    losses = []
    for _ in range(3):
        loss, ld = model.training_step_latents(z, cond, lr=1e-5, t=t, noise=noise)
        losses.append(loss.item())
        assert set(ld) == {"train_loss_simple", "train_loss"}
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[2] < losses[0], losses
    assert getattr(tr, "dctx", None) is None and model._cond_opt is None
    assert not torch.equal(model._ema_flat, ema0) and int(model.model_ema.num_updates) == 3
    if key == "adm":                    # the other forms apply_model accepts for the labels
        for form in ([cond], {"c_crossattn": [cond]}):
            loss, _ = model.p_losses(z, form, t, noise)
            assert np.isfinite(loss.item())
    else:
        loss, _ = model(z, None)
        assert np.isfinite(loss.item())


def test_latent_diffusion_concat_key_trains():
    """conditioning_key 'concat': the condition is concatenated on the channel axis, no context."""
    from dsml_thesis_amd import synth
    from dsml_thesis_amd.ddpm import LatentDiffusion
    cfg = synth.uncond_config(dict(UNCOND_SMALL, in_channels=7), synth.VQ_F4_256)
    cfg.update(cond_stage_config="__is_first_stage__", conditioning_key="concat")
    model = LatentDiffusion(**cfg)
    synth.load_recipe(model.model.diffusion_model, gain=0.5)
    model = model.cuda().train()
    assert model.model.conditioning_key == "concat"
    z, noise, t = rnd(90, 2, 4, 16, 16).cuda(), rnd(93, 2, 4, 16, 16).cuda(), torch.tensor([300, 800]).cuda()
    cat = rnd(94, 2, 3, 16, 16).cuda()
    losses = [model.training_step_latents(z, cat, lr=1e-5, t=t, noise=noise)[0].item() for _ in range(3)]
    assert all(np.isfinite(losses)) and losses[2] < losses[0], losses
    l_list, _ = model.p_losses(z, [cat], t, noise)
    l_dict, _ = model.p_losses(z, {"c_concat": [cat]}, t, noise)
    assert torch.equal(l_list, l_dict)


# ---- 10: bf16 compute ------------------------------------------------------------------------------------------------
def test_adm_bf16_training_step_gradients():
    """UNetTrainer(compute="bf16") on ADM_UNET with the bounds of test_bf16_training_step_gradients_against_float64_autograd:
    loss within 5e-3, relative L2 error per tensor <= 3e-2; no tensor of this UNet is dead, so none may be skipped."""
    from dsml_thesis_amd.train import reference_grad_layout
    cfg = W.ADM_UNET
    m, tr, sd, x0, noise, ctx, y, t = _setup(cfg, 3, 16, compute="bf16")
    loss_ref, grads, _, sched = _oracle_grads(cfg, sd, x0, noise, ctx, y, t, torch.float32)
    loss = _p_losses(tr, sched, x0, noise, ctx, y, t)
    print("bf16 loss", loss.item(), "reference", loss_ref.item())
    assert abs(loss.item() - loss_ref.item()) <= 5e-3 * abs(loss_ref.item()), (loss.item(), loss_ref.item())
    gdev = {k: (torch.zeros_like(sd[k]) if v is None else v.float()).cuda() for k, v in grads.items()}
    worst, skipped = (0.0, ""), 0
    for name, g in tr.P.g.items():
        ref = reference_grad_layout(m, name, gdev).double().cpu()
        nrm = ref.norm().item()
        if nrm < 1e-12:
            assert g.abs().max().item() == 0.0, name
            skipped += 1
            continue
        err = (g.double().cpu() - ref).norm().item() / nrm
        worst = max(worst, (err, name))
        assert err <= 3e-2, f"bf16 gradient {name}: relative L2 error {err:.3e}"
    print("worst bf16 gradient error", worst)
    assert skipped == 0, "ADM_UNET has no dead parameter tensor"
