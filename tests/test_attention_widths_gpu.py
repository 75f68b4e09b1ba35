"""GPU: every instantiation of the fp32 training attention (csrc/attention_train.hip) runs one arithmetic.  A head of 32
embedded in a head of 40, 64 or 80 whose other columns are zero must give the bits of the 32-wide entry point: the extra
MFMA steps and fmaf terms of the wider instantiation add exact zeros after the real ones, so equality is a property of the
arithmetic, not a tolerance.  Both sides get scale = 32 ** -0.5 (the `_d` entry points take the scale as an argument)."""
import pytest
import torch

from conftest import rnd

pytestmark = pytest.mark.gpu

N, HEADS, SCALE = 2, 2, 32 ** -0.5
WIDTHS = [40, 64, 80]


def _widen(x32, d):
    """[rows][k * 32] -> [rows][k * d]: columns [:32] of every head copied, the rest zero."""
    rows = x32.shape[0]
    wide = torch.zeros(rows, x32.shape[1] // 32, d, device=x32.device)
    wide[:, :, :32] = x32.view(rows, -1, 32)
    return wide.view(rows, -1)


def _check_embedded(got, ref32, d, what):
    """got [rows][k * d] against ref32 [rows][k * 32]: bitwise equal in columns [:32] of every head, zero in the rest."""
    g = got.view(got.shape[0], -1, d)
    same = torch.equal(g[:, :, :32], ref32.view(ref32.shape[0], -1, 32))
    zero = bool((g[:, :, 32:] == 0).all())
    print(f"{what} d={d}: columns [:32] bitwise equal {same}, columns [32:{d}] zero {zero}")
    assert same, f"{what}: d_head={d} differs from the 32-wide kernel"
    assert zero, f"{what}: d_head={d} wrote a non-zero into a padding column"


@pytest.mark.parametrize("tokens", [1, 33, 64, 129])
def test_self_attention_backward_is_one_arithmetic(tokens):
    from dsml_thesis_amd import lib as L
    from dsml_thesis_amd import ops
    from dsml_thesis_amd import train_ops as T
    C = HEADS * 32
    qkv32 = rnd(860, N * tokens, 3 * C).cuda()
    dout32 = rnd(861, N * tokens, C).cuda()
    out32, lse = T.attn_self_lse(qkv32, N, tokens, HEADS)
    dqkv32 = T.attn_self_bwd(qkv32, out32, dout32, lse, N, tokens, HEADS)
    assert torch.isfinite(dqkv32).all()
    p = lambda t: t.data_ptr()
    for d in WIDTHS:
        qkv, out, dout = _widen(qkv32, d), _widen(out32, d), _widen(dout32, d)
        dqkv = torch.full_like(qkv, float("nan"))
        dsum = torch.empty(N * HEADS * tokens, device="cuda")
        L.call("ldmk_attn_self_bwd_d", p(qkv), p(out), p(dout), p(lse), p(dqkv), p(dsum), N, tokens, HEADS, d, SCALE, ops.stream())
        _check_embedded(dqkv, dqkv32, d, f"d(qkv) tokens={tokens}")


@pytest.mark.parametrize("ctx_len", [1, 3, 77])
@pytest.mark.parametrize("tokens", [1, 65])
def test_cross_attention_backward_is_one_arithmetic(tokens, ctx_len):
    from dsml_thesis_amd import lib as L
    from dsml_thesis_amd import ops
    C = HEADS * 32
    q32, dout32 = rnd(862, N * tokens, C).cuda(), rnd(863, N * tokens, C).cuda()
    k32, v32 = rnd(864, N * ctx_len, C).cuda(), rnd(865, N * ctx_len, C).cuda()
    p = lambda t: t.data_ptr()

    def run(name, q, k, v, dout, *width):
        ld = q.shape[1]                                                  # compact rows
        dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
        scratch = torch.empty(2 * N * tokens * HEADS * ctx_len, device="cuda")
        L.call(name, p(q), ld, p(k), p(v), ld, p(dout), ld, p(dq), p(dk), p(dv), p(scratch), N, tokens, ctx_len, HEADS, *width,
               SCALE, ops.stream())
        return dq, dk, dv

    ref = run("ldmk_attn_cross_bwd", q32, k32, v32, dout32)
    assert all(torch.isfinite(t).all() for t in ref)
    for d in WIDTHS:
        got = run("ldmk_attn_cross_bwd_d", _widen(q32, d), _widen(k32, d), _widen(v32, d), _widen(dout32, d), d)
        for name, g, r in zip(("dq", "dk", "dv"), got, ref):
            _check_embedded(g, r, d, f"cross {name} tokens={tokens} ctx_len={ctx_len}")
