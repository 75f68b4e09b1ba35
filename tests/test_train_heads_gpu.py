"""GPU: training UNets whose attention heads are not 32 channels wide (csrc/attention_train.hip: ldmk_attn_self_lse_d,
ldmk_attn_self_bwd_d, ldmk_attn_cross_bwd_d) -- the kernels on their own at the tile edges, then whole-network gradients of
`p_losses` for H40_UNET (heads of 40 and 80), H64_UNET and AttentionBlock UNets with heads of 64.

References are float64 autograd on the CPU (float32 for the AttentionBlock UNets: the oracle casts to float32 inside its
GroupNorm32, see tests/test_train_variants_gpu.py).  Bounds are the existing ones: op level relative to max |ref| -- out 2e-5,
lse 1e-5, d(qkv) 3e-5, cross-attention gradients 3e-5 (tests/test_backward_edges_gpu.py); network level per parameter tensor
max |got - ref| / max |ref| <= 1e-4, loss 2e-5 against float64 (5e-5 against float32), context gradient 2e-4
(tests/test_train_variants_gpu.py).  The plain fp32 torch formula on the CPU stays at or below 1.0e-6 / 9.0e-8 / 1.1e-6 of
float64 for these widths (3.6e-6 / 3.5e-7 / 3.2e-6 with peaked rows), so the op-level bounds keep more than 4x margin over
the arithmetic.  Every test prints the figure it asserts on (run with -s)."""
import functools

import numpy as np
import pytest
import torch

from conftest import rnd
from oracle import ldm_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

SENT = 12345.0


@pytest.fixture(autouse=True)
def _autograd_on():
    """The reference side of these tests is autograd; other test modules switch it off process-wide."""
    with torch.enable_grad():
        yield


def _close(got, ref, rtol, what):
    from test_backward_edges_gpu import _close as close
    close(got, ref, rtol, what)


# ---------------------------------------------------------------------------------------------------------------------------
# 1-4. self attention, forward with log-sum-exp and flash backward
@functools.lru_cache(maxsize=None)
def _attn_ref(d, n, tokens, heads, qk_scale=1.0):
    """(qkv fp32, dout fp32, out, lse, d(qkv)) -- the last three float64 autograd of softmax(Q K^T / sqrt(d)) V."""
    C = heads * d
    qkv32 = rnd(830 + d, n * tokens, 3 * C)
    qkv32[:, :2 * C] *= qk_scale
    qkv = qkv32.double().requires_grad_(True)
    dout = rnd(831 + d, n * tokens, C)
    q, k, v = qkv.view(n, tokens, 3, heads, d).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) * d ** -0.5
    att = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(n * tokens, C)
    att.backward(dout.double())
    return qkv32, dout, att.detach(), torch.logsumexp(s, -1).detach(), qkv.grad


def _attn_run(d, n, tokens, heads, qkv, dout):
    """Forward and backward twice each (bitwise reproducible); the gradient goes into a NaN-filled buffer, so every element
    of all 3 C columns has to be written."""
    from dsml_thesis_amd import train_ops as T
    qd, dd = qkv.cuda(), dout.cuda()
    out, lse = T.attn_self_lse(qd, n, tokens, heads, d_head=d)
    out2, lse2 = T.attn_self_lse(qd, n, tokens, heads, d_head=d)
    assert torch.equal(out, out2) and torch.equal(lse, lse2), "attention forward must be bitwise reproducible"
    dqkv = torch.full_like(qd, float("nan"))
    again = torch.full_like(qd, float("nan"))
    assert T.attn_self_bwd(qd, out, dd, lse, n, tokens, heads, d_head=d, dqkv=dqkv) is dqkv
    T.attn_self_bwd(qd, out, dd, lse, n, tokens, heads, d_head=d, dqkv=again)
    unwritten = int((~torch.isfinite(dqkv)).sum().item())
    print(f"d_head={d} n={n} tokens={tokens} heads={heads}: {unwritten} of {dqkv.numel()} gradient elements not finite")
    assert unwritten == 0 and torch.isfinite(out).all() and torch.isfinite(lse).all()
    assert torch.equal(dqkv, again), "attention backward must be bitwise reproducible"
    assert out.shape == (n * tokens, heads * d) and lse.shape == (n, heads, tokens)
    return out, lse, dqkv


# token counts on the edges of the 32-key sub-tile, the 64-row staged tile and the 128-row workgroup
ATTN_EDGES = [(1, t, 2) for t in (1, 31, 33, 64, 65, 129)] + [(2, 65, 3)]


@pytest.mark.parametrize("n,tokens,heads", ATTN_EDGES)
@pytest.mark.parametrize("d", [40, 64, 80])
def test_self_attention_at_the_tile_edges(d, n, tokens, heads):
    qkv, dout, att, lse_ref, grad = _attn_ref(d, n, tokens, heads)
    out, lse, dqkv = _attn_run(d, n, tokens, heads, qkv, dout)
    _close(out, att, 2e-5, f"attention forward d={d}")
    _close(lse, lse_ref, 1e-5, f"log-sum-exp d={d}")
    _close(dqkv, grad, 3e-5, f"flash attention backward d={d}")


@pytest.mark.parametrize("d", [40, 80])
def test_self_attention_peaked_rows(d):
    """q and k scaled by 3: logits with a standard deviation near 9, most rows close to one-hot."""
    qkv, dout, att, lse_ref, grad = _attn_ref(d, 1, 129, 2, 3.0)
    out, lse, dqkv = _attn_run(d, 1, 129, 2, qkv, dout)
    _close(out, att, 2e-5, f"peaked attention forward d={d}")
    _close(lse, lse_ref, 1e-5, f"peaked log-sum-exp d={d}")
    _close(dqkv, grad, 3e-5, f"peaked flash attention backward d={d}")


def test_self_attention_rows_do_not_depend_on_the_batch():
    """A ragged count (65): appending a second sample must not change a bit of the first sample's rows."""
    qkv, dout, *_ = _attn_ref(40, 2, 65, 3)
    out2, lse2, d2 = _attn_run(40, 2, 65, 3, qkv, dout)
    out1, lse1, d1 = _attn_run(40, 1, 65, 3, qkv[:65].contiguous(), dout[:65].contiguous())
    same = [torch.equal(out1, out2[:65]), torch.equal(lse1[0], lse2[0]), torch.equal(d1, d2[:65])]
    print("first sample bitwise equal (out, lse, dqkv):", same)
    assert all(same)


def test_self_attention_keeps_no_score_matrix_in_memory():
    """2048 tokens, 2 heads of 64: a materialised [heads][T][T] fp32 score matrix is 33.5 MB; forward plus backward may raise
    the allocator's peak by less than half of that."""
    from dsml_thesis_amd import train_ops as T
    d, n, tokens, heads = 64, 1, 2048, 2
    qkv, dout, att, lse_ref, grad = _attn_ref(d, n, tokens, heads)
    qd, dd = qkv.cuda(), dout.cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, lse = T.attn_self_lse(qd, n, tokens, heads, d_head=d)
    dqkv = T.attn_self_bwd(qd, out, dd, lse, n, tokens, heads, d_head=d)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    limit = heads * tokens * tokens * 4 // 2
    print(f"peak allocation rose by {rise / 2 ** 20:.2f} MB (limit {limit / 2 ** 20:.2f} MB)")
    assert rise < limit
    _close(out, att, 2e-5, "attention forward, 2048 tokens")
    _close(lse, lse_ref, 1e-5, "log-sum-exp, 2048 tokens")
    _close(dqkv, grad, 3e-5, "flash attention backward, 2048 tokens")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. cross-attention backward with leading dimensions
@pytest.mark.parametrize("L_ctx", [1, 3, 77])
@pytest.mark.parametrize("d", [40, 64, 80])
def test_cross_attention_backward_strided(d, L_ctx):
    """q, k, v, dout and the gradients as column slices of wider sentinel-filled buffers: gradients within 3e-5 of float64
    autograd, the other columns untouched, values bitwise those of the contiguous call."""
    from dsml_thesis_amd import train_ops as T
    n, tokens, heads = 2, 37, 2
    C_ = heads * d
    q = rnd(840, n * tokens, C_).double().requires_grad_(True)
    k = rnd(841, n * L_ctx, C_).double().requires_grad_(True)
    v = rnd(842, n * L_ctx, C_).double().requires_grad_(True)
    qh = q.view(n, tokens, heads, d).permute(0, 2, 1, 3)
    kh = k.view(n, L_ctx, heads, d).permute(0, 2, 1, 3)
    vh = v.view(n, L_ctx, heads, d).permute(0, 2, 1, 3)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * d ** -0.5, -1)
    out = (p @ vh).permute(0, 2, 1, 3).reshape(n * tokens, C_)
    dout = rnd(843, n * tokens, C_)
    out.backward(dout.double())
    wq, wkv = C_ + 32, 2 * C_ + 32
    qbuf, kvbuf, dobuf = (torch.full(s, 3.0, device="cuda") for s in ((n * tokens, wq), (n * L_ctx, wkv), (n * tokens, wq)))
    qs, ks, vs, dos = qbuf[:, :C_], kvbuf[:, :C_], kvbuf[:, C_:2 * C_], dobuf[:, 16:16 + C_]
    qs.copy_(q.detach().float()); ks.copy_(k.detach().float()); vs.copy_(v.detach().float()); dos.copy_(dout)
    dqbuf, dkvbuf = torch.full((n * tokens, wq), SENT, device="cuda"), torch.full((n * L_ctx, wkv), SENT, device="cuda")
    dq, dk, dv = T.attn_cross_bwd(qs, ks, vs, dos, n, tokens, L_ctx, heads, dq=dqbuf[:, :C_], dk=dkvbuf[:, :C_],
                                  dv=dkvbuf[:, C_:2 * C_], d_head=d)
    _close(dq, q.grad, 3e-5, f"strided cross attention dq d={d} L={L_ctx}")
    _close(dk, k.grad, 3e-5, f"strided cross attention dk d={d} L={L_ctx}")
    _close(dv, v.grad, 3e-5, f"strided cross attention dv d={d} L={L_ctx}")
    intact = bool((dqbuf[:, C_:] == SENT).all() and (dkvbuf[:, 2 * C_:] == SENT).all())
    print("sentinel columns intact:", intact)
    assert intact, "columns outside the gradient slices were written"
    assert bool((qbuf[:, C_:] == 3.0).all() and (kvbuf[:, 2 * C_:] == 3.0).all()), "an input buffer was written"
    dq3, dk3, dv3 = T.attn_cross_bwd(qs.contiguous(), ks.contiguous(), vs.contiguous(), dos.contiguous(), n, tokens, L_ctx, heads,
                                     d_head=d)
    same = [dq3.is_contiguous(), torch.equal(dq3, dq), torch.equal(dk3, dk), torch.equal(dv3, dv)]
    print("contiguous call bitwise equal:", same)
    assert all(same)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. rejections
@pytest.mark.parametrize("d", [36 + 2, 100, 32])
def test_entry_points_reject_unsupported_head_widths(d):
    from dsml_thesis_amd import lib as L
    from dsml_thesis_amd import ops
    n, tokens, heads, L_ctx = 1, 8, 2, 3
    buf = lambda *s: torch.zeros(*s, device="cuda")
    C_ = heads * d
    qkv, out, lse, dsum = buf(n * tokens, 3 * C_), buf(n * tokens, C_), buf(n, heads, tokens), buf(n * heads * tokens)
    p = lambda t: t.data_ptr()
    with pytest.raises(L.LdmkError, match="head width"):
        L.call("ldmk_attn_self_lse_d", p(qkv), p(out), p(lse), n, tokens, heads, d, d ** -0.5, ops.stream())
    with pytest.raises(L.LdmkError, match="head width"):
        L.call("ldmk_attn_self_bwd_d", p(qkv), p(out), p(out), p(lse), p(torch.empty_like(qkv)), p(dsum), n, tokens, heads, d,
               d ** -0.5, ops.stream())
    k = buf(n * L_ctx, C_)
    with pytest.raises(L.LdmkError, match="head width"):
        L.call("ldmk_attn_cross_bwd_d", p(out), C_, p(k), p(k), C_, p(out), C_, p(buf(n * tokens, C_)), p(buf(n * L_ctx, C_)),
               p(buf(n * L_ctx, C_)), p(buf(2 * n * tokens * heads * L_ctx)), n, tokens, L_ctx, heads, d, d ** -0.5, ops.stream())
    print(f"d_head={d}: all three _d entry points raised LdmkError")


def test_trainer_names_an_unsupported_head_width():
    from dsml_thesis_amd.train import UNetTrainer
    from dsml_thesis_amd.unet import UNetModel
    cfg = dict(W.ADM_UNET, model_channels=96, num_head_channels=48)
    m = UNetModel(**cfg)
    m.load_state_dict(W.synth_state_dict(W.unet_param_shapes(cfg)), strict=True)
    with pytest.raises(NotImplementedError, match="48") as e:
        UNetTrainer(m.cuda().eval())
    print("refusal:", e.value)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. whole-network gradients of p_losses
def _network(cfg, n, hw, L_ctx, compute="f32"):
    from test_train_variants_gpu import _setup
    m, tr, sd, x0, noise, ctx, y, t = _setup(cfg, n, hw, compute=compute)
    if ctx is not None and L_ctx != 1:
        ctx = rnd(3, n, L_ctx, cfg["context_dim"])
    return m, tr, sd, x0, noise, ctx, y, t


def _check(cfg, n, hw, dtype, loss_rtol, L_ctx=1):
    from test_train_gpu import _check_all_grads
    from test_train_variants_gpu import _oracle_grads, _p_losses
    m, tr, sd, x0, noise, ctx, y, t = _network(cfg, n, hw, L_ctx)
    widths = sorted({mod.d_head for _, mod in m._walk() if mod.kind in ("st", "attn")})
    loss_ref, grads, dctx_ref, sched = _oracle_grads(cfg, sd, x0, noise, ctx, y, t, dtype)
    loss = _p_losses(tr, sched, x0, noise, ctx, y, t)
    rel = abs(loss.item() - loss_ref.item()) / abs(loss_ref.item())
    print("head widths", widths, "loss", loss.item(), "reference", loss_ref.item(), "relative", rel)
    assert rel <= loss_rtol, (loss.item(), loss_ref.item())
    worst = _check_all_grads(m, tr, grads, 1e-4)
    print("worst gradient error", worst)
    if ctx is not None:
        err = (tr.dctx.double().cpu() - dctx_ref.reshape(tr.dctx.shape)).abs().max().item() / dctx_ref.abs().max().item()
        print("context gradient error", err)
        assert err <= 2e-4, f"context gradient {err:.3e}"
    return widths


@pytest.mark.parametrize("L_ctx", [1, 3])
@pytest.mark.parametrize("tag", ["h40", "h64"])
def test_spatial_transformer_unet_gradients_float64(tag, L_ctx):
    """H40_UNET (heads of 40 at 160 channels, 80 at 320) and H64_UNET, n = 2, 16x16.  One context token: the single-token
    short-cut; three: ldmk_attn_cross_d forward and ldmk_attn_cross_bwd_d inside the tape."""
    cfg = dict(h40=W.H40_UNET, h64=W.H64_UNET)[tag]
    widths = _check(cfg, 2, 16, torch.float64, 2e-5, L_ctx)
    assert widths == dict(h40=[40, 80], h64=[64])[tag]


def test_adm_unet_gradients_new_order_attention_heads_of_64():
    """AttentionBlock with use_new_attention_order, heads of 64, n = 3 with labels; float32 oracle."""
    assert _check(dict(W.ADM_UNET, num_head_channels=64), 3, 16, torch.float32, 5e-5) == [64]


def test_unconditional_unet_gradients_legacy_attention_order_heads_of_64():
    """AttentionBlock / QKVAttentionLegacy ([head][q | k | v][d] qkv rows), heads of 64; float32 oracle."""
    from test_train_variants_gpu import UNCOND_SMALL
    assert _check(dict(UNCOND_SMALL, num_head_channels=64), 2, 16, torch.float32, 5e-5) == [64]


# ---------------------------------------------------------------------------------------------------------------------------
# 8. training forward == sampling forward
@pytest.mark.parametrize("tag", ["h40", "h64"])
def test_training_forward_matches_sampling_forward(tag):
    cfg = dict(h40=W.H40_UNET, h64=W.H64_UNET)[tag]
    m, tr, sd, x0, noise, ctx, y, t = _network(cfg, 2, 16, 1)
    eps_t = tr.forward(x0.cuda(), t.cuda(), ctx.cuda())
    eps_s = m(x0.cuda(), t.cuda(), context=ctx.cuda())
    print("max |training - sampling|", (eps_t - eps_s).abs().max().item(), "max |eps|", eps_s.abs().max().item())
    torch.testing.assert_close(eps_t, eps_s, rtol=2e-4, atol=2e-5)


# ---------------------------------------------------------------------------------------------------------------------------
# 9. bf16 compute mode
def test_bf16_training_step_heads_of_64():
    """UNetTrainer(compute="bf16") on H64_UNET at the bounds of test_bf16_training_step_gradients_against_float64_autograd:
    loss within 5e-3, relative L2 error per parameter tensor <= 3e-2 (dead tensors exactly zero); two AdamW steps lower the
    loss.  The attention of these widths runs on the fp32 kernels in this mode."""
    from test_train_variants_gpu import _oracle_grads, _p_losses
    from dsml_thesis_amd.train import reference_grad_layout
    cfg = W.H64_UNET
    m, tr, sd, x0, noise, ctx, y, t = _network(cfg, 2, 16, 1, compute="bf16")
    loss_ref, grads, _, sched = _oracle_grads(cfg, sd, x0, noise, ctx, y, t, torch.float64)
    loss = _p_losses(tr, sched, x0, noise, ctx, y, t)
    print("bf16 loss", loss.item(), "reference", loss_ref.item())
    assert abs(loss.item() - loss_ref.item()) <= 5e-3 * abs(loss_ref.item()), (loss.item(), loss_ref.item())
    gdev = {k: (torch.zeros_like(sd[k]) if v is None else v.float()).cuda() for k, v in grads.items()}
    worst = (0.0, "")
    for name, g in tr.P.g.items():
        ref = reference_grad_layout(m, name, gdev).double().cpu()
        nrm = ref.norm().item()
        if nrm < 1e-12:
            assert g.abs().max().item() == 0.0, name          # dead branches stay exactly zero
            continue
        err = (g.double().cpu() - ref).norm().item() / nrm
        worst = max(worst, (err, name))
        assert err <= 3e-2, f"bf16 gradient {name}: relative L2 error {err:.3e}"
    print("worst bf16 gradient error", worst)
    losses = [loss.item()]
    for _ in range(2):
        tr.adamw_step(lr=2e-5)
        losses.append(_p_losses(tr, sched, x0, noise, ctx, y, t).item())
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


# ---------------------------------------------------------------------------------------------------------------------------
# 10. differentiable DDIM: the gradient with respect to the network input
def test_input_gradient_heads_of_64():
    """UNetTrainer(want_dx=True) on H64_UNET: d(sum(eps o g))/d(x) of one forward and backward against float64 autograd on the
    oracle, at the 1e-4 (relative to max |ref|) of the op-level input-gradient check of the differentiable decode."""
    from dsml_thesis_amd.train import UNetTrainer
    cfg = W.H64_UNET
    m, _, sd, x0, noise, ctx, y, t = _network(cfg, 2, 16, 1)
    tr = UNetTrainer(m, want_dx=True)
    g = rnd(850, *noise.shape)
    eps = tr.forward(x0.cuda(), t.cuda(), ctx.cuda())
    dx = tr.backward(tr.pad_output_grad(g.cuda()))
    x = x0.double().requires_grad_(True)
    ref = O.unet_forward({k: v.double() for k, v in sd.items()}, cfg, x, t, ctx.double())
    ref.backward(g.double())
    torch.testing.assert_close(eps.cpu().double(), ref.detach(), rtol=2e-4, atol=2e-5)
    assert dx is not None and dx.shape == x0.shape
    err = (dx.cpu().double() - x.grad).abs().max().item() / x.grad.abs().max().item()
    print("input gradient error", err)
    assert err <= 1e-4, f"input gradient: {err:.3e}"
