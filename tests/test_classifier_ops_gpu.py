"""Op-level parity of the pooled-head kernels and the cross-entropy (csrc/classifier.hip) against the same operation in float64 on
the CPU, built from the fp32 inputs.

Metrics -- those the project's op-level float64 parity tests already hold kernels of the same kind to, no new number:
  sums kept in double and rounded once (means, losses)   assert_close rtol 1e-6 / atol 0   (test_objective_ops_gpu.py)
  sums with one further fp32 addition                    max|got - ref| <= 2e-5 max|ref|   (`_close`, test_small_ops_gpu.py: sums)
  softmax and what is built on it                        assert_close rtol 1e-4 / atol 1e-5 (test_small_ops_gpu.py: softmax)
  data moves / plain fp32 additions                      torch.equal
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    from dsml_thesis_amd import lib, train_ops
    lib.load()
    return train_ops


def _close(got, ref, rtol, what):
    ref = ref.to(torch.float64)
    err = (got.detach().cpu().to(torch.float64) - ref).abs().max().item()
    bound = rtol * max(ref.abs().max().item(), 1e-30)
    print(f"{what}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def _assert_close(got, ref, rtol, atol):
    torch.testing.assert_close(got.detach().cpu().double(), ref.double(), rtol=rtol, atol=atol)


# ------------------------------------------------------------------------------------------ pool mean
POOL_SHAPES = [(1, 1, 32), (3, 49, 160), (3, 64, 128), (2, 4096, 160)]


@pytest.mark.parametrize("n,hw,c", POOL_SHAPES)
def test_pool_mean_forward(T, n, hw, c):
    x = rnd(11 + hw, n, hw, c)
    ld, col = c + 40, 24                                  # col != 0, ld > c: the other columns keep their sentinel
    feat = torch.full((n, ld), -777.25, device="cuda")
    T.pool_mean(x.cuda(), n, hw, feat=feat, col=col)
    _assert_close(feat[:, col:col + c], x.double().mean(1), 1e-6, 0)
    assert bool((feat[:, :col] == -777.25).all()) and bool((feat[:, col + c:] == -777.25).all())
    fresh = T.pool_mean(x.cuda(), n, hw)
    assert torch.equal(fresh, feat[:, col:col + c]) and torch.equal(T.pool_mean(x.cuda(), n, hw), fresh)


def test_pool_mean_of_a_mean_dominated_input(T):
    """mean 100, sigma 1: the spread of the means (~1 / 8 here) has to survive under the mean itself."""
    x = 100.0 + rnd(12, 3, 64, 128)
    got = T.pool_mean(x.cuda(), 3, 64)
    ref = x.double().mean(1)
    _assert_close(got, ref, 1e-6, 0)
    _close(got.cpu().double() - 100.0, ref - 100.0, 2e-5, "deviation of the means from 100")


@pytest.mark.parametrize("n,hw,c", POOL_SHAPES)
def test_pool_mean_backward(T, n, hw, c):
    ld, col = c + 40, 24
    dfeat = rnd(13 + hw, n, ld)
    ref = (dfeat[:, col:col + c].double() / hw)[:, None, :].expand(n, hw, c)
    dx = T.pool_mean_bwd(dfeat.cuda(), n, hw, c, col=col)
    _assert_close(dx, ref, 1e-6, 0)
    prev = rnd(14 + hw, n, hw, c)
    acc = prev.cuda()
    T.pool_mean_bwd(dfeat.cuda(), n, hw, c, col=col, dx=acc, accumulate=True)
    _close(acc, prev.double() + ref, 2e-5, "pool_mean_bwd accumulate")
    assert torch.equal(acc.cpu(), prev + dx.cpu())        # one fp32 addition on top of the plain result


def test_pool_mean_rejects_columns_outside_the_row(T):
    x = torch.zeros(2, 4, 32, device="cuda")
    with pytest.raises(ValueError):
        T.pool_mean(x, 2, 4, feat=torch.zeros(2, 40, device="cuda"), col=16)


# ------------------------------------------------------------------------------------------ token rows
@pytest.mark.parametrize("hw", [1, 4, 64])
def test_attnpool_tokens_forward_and_backward(T, hw):
    n, c = 3, 96
    y, pos_t = rnd(21 + hw, n, hw, c), rnd(22 + hw, hw + 1, c)
    X = T.attnpool_tokens(y.cuda().view(n * hw, c), pos_t.cuda(), n, hw).view(n, hw + 1, c)
    ref = torch.cat([y.double().mean(1, keepdim=True), y.double()], 1) + pos_t.double()
    _close(X, ref, 2e-5, "token rows")
    assert torch.equal(X[:, 1:].cpu(), y + pos_t[1:])     # the pixel rows are one fp32 addition
    assert torch.equal(T.attnpool_tokens(y.cuda().view(n * hw, c), pos_t.cuda(), n, hw).view(n, hw + 1, c), X)

    dX = rnd(23 + hw, n, hw + 1, c)
    dy, dpos = T.attnpool_tokens_bwd(dX.cuda().view(n * (hw + 1), c), n, hw)
    _close(dy.view(n, hw, c), dX[:, 1:].double() + dX[:, :1].double() / hw, 2e-5, "dy")
    _assert_close(dpos, dX.double().sum(0), 1e-6, 1e-30)  # summed over the n = 3 samples in double, rounded once
    dy2, dpos2 = T.attnpool_tokens_bwd(dX.cuda().view(n * (hw + 1), c), n, hw)
    assert torch.equal(dy, dy2) and torch.equal(dpos, dpos2)
    acc = rnd(24 + hw, hw + 1, c)
    got = acc.cuda()
    T.attnpool_tokens_bwd(dX.cuda().view(n * (hw + 1), c), n, hw, dpos_t=got, accumulate=True, want_dy=False)
    assert torch.equal(got.cpu(), acc + dpos.cpu())


# ------------------------------------------------------------------------------------------ single-query attention
def _attnpool_ref(qkv, n, Tk, heads, d):
    """float64 autograd through the reference's formulation: q and k each scaled by d^-1/4, softmax over the keys, token 0 only."""
    C_ = heads * d
    x = qkv.double().view(n, Tk, 3, heads, d).requires_grad_(True)
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    s = d ** -0.25
    w = torch.einsum("nhd,nthd->nht", q[:, 0] * s, k * s)
    p = torch.softmax(w, -1)
    out = torch.einsum("nht,nthd->nhd", p, v).reshape(n, C_)
    return x, p, out


APOOL_CASES = [(Tk, 32, heads, n) for Tk, heads, n in ((2, 1, 1), (5, 4, 3), (65, 4, 3), (257, 1, 3), (1025, 4, 1))] + \
              [(65, d, heads, n) for d, heads, n in ((40, 4, 3), (64, 1, 3), (80, 4, 1))]


@pytest.mark.parametrize("Tk,d,heads,n", APOOL_CASES)
def test_attnpool_forward_and_backward(T, Tk, d, heads, n):
    C_ = heads * d
    qkv = rnd(31 + Tk + d, n * Tk, 3 * C_)
    dout = rnd(32 + Tk + d, n, C_)
    with torch.enable_grad():
        x, p_ref, out_ref = _attnpool_ref(qkv, n, Tk, heads, d)
        (out_ref * dout.double()).sum().backward()
    out, probs = T.attnpool_fwd(qkv.cuda(), n, Tk, heads, d)
    _assert_close(out, out_ref.detach(), 1e-4, 1e-5)
    _assert_close(probs, p_ref.detach(), 1e-4, 1e-5)
    _assert_close(probs.sum(-1), torch.ones(n, heads), 1e-6, 0)
    dqkv = T.attnpool_bwd(qkv.cuda(), probs, dout.cuda(), n, Tk, heads, d)
    _assert_close(dqkv, x.grad.view(n * Tk, 3 * C_), 1e-4, 1e-5)
    dq = dqkv.view(n, Tk, 3, C_)[:, 1:, 0]
    assert dq.numel() == 0 or bool((dq == 0).all())        # the q columns of every token but 0: exact zeros
    out2, probs2 = T.attnpool_fwd(qkv.cuda(), n, Tk, heads, d)
    assert torch.equal(out, out2) and torch.equal(probs, probs2)
    assert torch.equal(dqkv, T.attnpool_bwd(qkv.cuda(), probs, dout.cuda(), n, Tk, heads, d))


def test_attnpool_with_one_key_far_above_the_rest(T):
    """Key 3's logit sits 60 above the others: the max subtraction keeps the softmax finite and the output is v_3."""
    n, Tk, heads, d = 1, 65, 1, 32
    qkv = 0.01 * rnd(33, n * Tk, 3 * d)
    qkv[0, :d] = 1.0
    qkv[3, d:2 * d] = 60.0 * d ** 0.5 / d                   # q_0 . k_3 d^-1/2 = 60
    dout = rnd(34, n, d)
    with torch.enable_grad():
        x, p_ref, out_ref = _attnpool_ref(qkv, n, Tk, heads, d)
        (out_ref * dout.double()).sum().backward()
    assert 59.0 < float((p_ref[0, 0, 3] / p_ref[0, 0, 4]).log()) < 61.0
    out, probs = T.attnpool_fwd(qkv.cuda(), n, Tk, heads, d)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(probs).all())
    _assert_close(out, out_ref.detach(), 1e-4, 1e-5)
    _assert_close(probs, p_ref.detach(), 1e-4, 1e-5)
    dqkv = T.attnpool_bwd(qkv.cuda(), probs, dout.cuda(), n, Tk, heads, d)
    _assert_close(dqkv, x.grad.view(n * Tk, 3 * d), 1e-4, 1e-5)


def test_attnpool_validates_its_shapes(T):
    from dsml_thesis_amd import lib as L
    with pytest.raises(L.LdmkError, match="d_head"):
        T.attnpool_fwd(torch.zeros(2, 3 * 6, device="cuda"), 1, 2, 1, 6)
    with pytest.raises(L.LdmkError, match="tokens above"):
        T.attnpool_fwd(torch.zeros(4097, 3 * 32, device="cuda"), 1, 4097, 1, 32)


# ------------------------------------------------------------------------------------------ cross-entropy
@pytest.mark.parametrize("K", [2, 8, 1000])
@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("offset", [0.0, 80.0, -80.0])
def test_cross_entropy(T, K, n, offset):
    logits = rnd(41 + K + n, n, K) + offset
    y = torch.from_numpy(np.random.RandomState(42 + K + n).randint(0, K, size=n).astype(np.int64))
    y[0] = 0
    y[-1] = K - 1
    ref_per = F.cross_entropy(logits.double(), y, reduction="none")
    ref_dl = (torch.softmax(logits.double(), -1) - F.one_hot(y, K).double())
    per, mean, dl = T.cross_entropy(logits.cuda(), y.cuda())
    _assert_close(per, ref_per, 1e-6, 0)
    _assert_close(mean, ref_per.mean().view(1), 1e-6, 0)
    _assert_close(dl, ref_dl / n, 1e-4, 1e-5)
    assert float(dl.double().sum(-1).abs().max()) <= 1e-6
    per2, mean2, none = T.cross_entropy(logits.cuda(), y.cuda(), want_dlogits=False)
    assert none is None and torch.equal(per, per2) and torch.equal(mean, mean2)
    _, _, neg = T.cross_entropy(logits.cuda(), y.cuda(), scale=-1.0)          # onehot - softmax: the guidance direction
    _assert_close(neg, -ref_dl, 1e-4, 1e-5)


def test_cross_entropy_validates_on_the_host(T):
    with pytest.raises(ValueError, match="K <= 1024"):
        T.cross_entropy(torch.zeros(2, 1025, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="int64"):
        T.cross_entropy(torch.zeros(2, 8, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------------------------------ ReLU, GroupNorm of one pixel
def test_relu_forward_and_backward(T):
    x, dy = rnd(51, 5, 2048), rnd(52, 5, 2048)
    x[0, :4] = torch.tensor([0.0, -0.0, 1e-30, -1e-30])
    assert torch.equal(T.relu(x.cuda()).cpu(), torch.relu(x))
    assert torch.equal(T.relu_bwd(x.cuda(), dy.cuda()).cpu(), torch.where(x > 0, dy, torch.zeros_like(dy)))


def test_groupnorm_of_one_pixel_rows(T):
    """spatial_v2 normalises a (n, 2048) matrix: 32 groups of 64 channels, hw = 1.  The existing GroupNorm kernels take it; held
    to the sums bound of the project's GroupNorm tests' kind (max-relative 2e-5 forward and backward)."""
    from dsml_thesis_amd import lib as L, ops
    n, c = 3, 2048
    x, gamma, beta, dy = rnd(61, n, c), 1 + 0.1 * rnd(62, c), 0.1 * rnd(63, c), rnd(64, n, c)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    part = torch.empty(n * L.load().ldmk_gn_chunks(1) * c * 3, device="cuda")
    L.call("ldmk_gn_partial", xd.data_ptr(), c, n, 1, part.data_ptr(), ops.stream())
    coef = torch.empty(n, 2, c, device="cuda")
    L.call("ldmk_gn_finalize", part.data_ptr(), c, 0, 0, n, 1, 32, 1e-5, gd.data_ptr(), bd.data_ptr(), coef.data_ptr(), ops.stream())
    mr = T.gn_group_stats(part, c, None, 0, n, 1, 32, 1e-5)
    y = ops.gn_apply(xd, None, coef, n, 1, silu=True)
    with torch.enable_grad():
        x64 = x.double().requires_grad_(True)
        g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        ref = F.silu(F.group_norm(x64, 32, g64, b64, 1e-5))
        (ref * dy.double()).sum().backward()
    _close(y, ref.detach(), 2e-5, "GroupNorm + SiLU, hw = 1")
    dx, _, dgamma, dbeta = T.gn_bwd(xd, None, dy.cuda(), coef, mr, gd, n, 1, silu=True)
    _close(dx, x64.grad, 2e-5, "dx")
    _close(dgamma, g64.grad, 2e-5, "dgamma")
    _close(dbeta, b64.grad, 2e-5, "dbeta")
