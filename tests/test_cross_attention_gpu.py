"""Op-level parity of the short-context cross attention (ldmk_attn_cross / ldmk_attn_cross_d, csrc/attention.hip) against
float64 softmax(q k^T / sqrt(d)) v on the CPU, built from the fp32 inputs: every built head width, contexts from one key
to the 128-key limit, leading dimensions wider than heads * d on q, k / v and out, totals below one 256-thread workgroup
and ragged above it, and a dominating key that makes the running maximum jump (first key: everything after it is
rescaled against it; last key: the whole accumulated sum is rescaled at the end).

Metric: max|got - ref| <= 2e-5 * max|ref|, the bound tests/test_backward_gpu.py states for the attention forward.  It was
checked on the CPU to hold for a plain fp32 torch evaluation of the same formula at these inputs."""
import pytest
import torch

from conftest import rnd

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
SHAPES = [(2, 37, 3), (1, 300, 2)]          # (n, tokens, heads): 222 threads < one workgroup; 600 = 2 workgroups + 88


@pytest.fixture(scope="module")
def ops():
    from dsml_thesis_amd import ops as ops_
    from dsml_thesis_amd import lib
    lib.load()
    return ops_


def _close(got, ref, rtol, what):
    ref = ref.to(torch.float64)
    err = (got.detach().cpu().to(torch.float64) - ref).abs().max().item()
    bound = rtol * max(ref.abs().max().item(), 1e-30)
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def cross_inputs(d, L_ctx, n, tokens, heads, spike=None):
    """(q wide, k wide, v wide): q lives in columns [4, 4 + heads d) of a [n tokens][heads d + 8] tensor, k and v in the
    first heads d columns of [n L][heads d + 4] tensors; q and k are scaled by 2 (logits ~ N(0, 16): a peaky softmax).
    spike = 'first' / 'last': every query and that key share a large first component per head, which puts the key's logit
    256 / sqrt(d) (28 to 45) above the others'."""
    C_ = heads * d
    seed = 9000 + 13 * d + L_ctx + tokens
    qw, kw, vw = 2.0 * rnd(seed, n * tokens, C_ + 8), 2.0 * rnd(seed + 1, n * L_ctx, C_ + 4), rnd(seed + 2, n * L_ctx, C_ + 4)
    if spike is not None:
        j = 0 if spike == "first" else L_ctx - 1
        qw[:, 4:4 + C_:d] = 8.0
        kw[:, 0:C_:d] = 0.0
        kw.view(n, L_ctx, C_ + 4)[:, j, 0:C_:d] = 32.0
    return qw, kw, vw


def cross_ref(qw, kw, vw, d, L_ctx, n, tokens, heads, dtype=torch.float64):
    C_ = heads * d
    q = qw[:, 4:4 + C_].to(dtype).view(n, tokens, heads, d).permute(0, 2, 1, 3)
    k = kw[:, :C_].to(dtype).view(n, L_ctx, heads, d).permute(0, 2, 1, 3)
    v = vw[:, :C_].to(dtype).view(n, L_ctx, heads, d).permute(0, 2, 1, 3)
    p = torch.softmax(q @ k.transpose(-1, -2) * (d ** -0.5), -1)
    return (p @ v).permute(0, 2, 1, 3).reshape(n * tokens, C_)


def _run(ops, qw, kw, vw, d, L_ctx, n, tokens, heads, d_head):
    C_ = heads * d
    qd, kd, vd = qw.cuda(), kw.cuda(), vw.cuda()
    wide = torch.full((n * tokens, C_ + 12), SENTINEL, device="cuda")
    out = wide[:, :C_]
    q, k, v = qd[:, 4:4 + C_], kd[:, :C_], vd[:, :C_]
    assert q.stride(0) > C_ and k.stride(0) > C_ and out.stride(0) > C_ and k.stride(0) == v.stride(0)
    ops.attn_cross(q, k, v, n, tokens, L_ctx, heads, out=out, d_head=d_head)
    assert torch.all(wide[:, C_:] == SENTINEL), "wrote into the padding columns of out"
    return out


@pytest.mark.parametrize("n,tokens,heads", SHAPES)
@pytest.mark.parametrize("L_ctx", [1, 2, 77, 128])
@pytest.mark.parametrize("d", [32, 40, 64, 80])
def test_attn_cross_float64(ops, d, L_ctx, n, tokens, heads):
    """ldmk_attn_cross_d at head widths 32 / 40 / 64 / 80 (and ldmk_attn_cross, which must give the same bits at 32) against
    the float64 attention; ldq, ldkv, ldo > heads * d with the padding of out untouched; bound 2e-5 * max|ref|."""
    qw, kw, vw = cross_inputs(d, L_ctx, n, tokens, heads)
    ref = cross_ref(qw, kw, vw, d, L_ctx, n, tokens, heads)
    out = _run(ops, qw, kw, vw, d, L_ctx, n, tokens, heads, d)
    _close(out, ref, 2e-5, f"attn_cross_d d={d} L={L_ctx} n={n} tokens={tokens} heads={heads}")
    if d == 32:
        out32 = _run(ops, qw, kw, vw, d, L_ctx, n, tokens, heads, None)
        assert torch.equal(out32, out), "ldmk_attn_cross differs from ldmk_attn_cross_d(32)"


@pytest.mark.parametrize("spike", ["first", "last"])
@pytest.mark.parametrize("d", [32, 40, 64, 80])
def test_attn_cross_dominating_key(ops, d, spike):
    """One key 28 to 45 logits above the other 127, at index 0 and at index L - 1 (the running maximum jumps on the last
    key and the whole accumulator is rescaled by about exp(-28) or less); same reference and bound."""
    n, tokens, heads, L_ctx = 1, 300, 2, 128
    qw, kw, vw = cross_inputs(d, L_ctx, n, tokens, heads, spike=spike)
    ref = cross_ref(qw, kw, vw, d, L_ctx, n, tokens, heads)
    out = _run(ops, qw, kw, vw, d, L_ctx, n, tokens, heads, None if d == 32 else d)
    _close(out, ref, 2e-5, f"attn_cross dominating key {spike} d={d}")


def test_attn_cross_rejections(ops):
    """Refused before any launch: L = 0, L = 129, d = 48, and a leading dimension of q, k / v or out that is no multiple of
    4.  Every buffer is valid memory, large enough for the call as stated."""
    from dsml_thesis_amd import lib as L
    n, tokens, heads = 1, 8, 2
    q = torch.zeros(n * tokens, heads * 48 + 2, device="cuda")
    kv = torch.zeros(n * 129, heads * 48 + 2, device="cuda")
    out = torch.zeros(n * tokens, heads * 48 + 2, device="cuda")
    q4, kv4, out4 = q[:, :96].contiguous(), kv[:, :96].contiguous(), out[:, :96].contiguous()
    with pytest.raises(L.LdmkError, match="ctx_len=0"):
        ops.attn_cross(q4, kv4, kv4, n, tokens, 0, heads, out=out4, d_head=32)
    with pytest.raises(L.LdmkError, match="ctx_len=129"):
        ops.attn_cross(q4, kv4, kv4, n, tokens, 129, heads, out=out4, d_head=32)
    with pytest.raises(L.LdmkError, match="head width 48"):
        ops.attn_cross(q4, kv4, kv4, n, tokens, 77, heads, out=out4, d_head=48)
    for bad in range(3):                     # ldq, ldkv, ldo = 98 in turn; the other two are 96
        args = [q[:, :64] if bad == 0 else q4, kv[:, :64] if bad == 1 else kv4, out[:, :64] if bad == 2 else out4]
        with pytest.raises(L.LdmkError, match="multiples of 4"):
            ops.attn_cross(args[0], args[1], args[1], n, tokens, 77, heads, out=args[2], d_head=32)
    ops.attn_cross(q4, kv4, kv4, n, tokens, 128, heads, out=out4, d_head=32)       # the accepted neighbour
    torch.cuda.synchronize()
