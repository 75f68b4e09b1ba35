"""CPU: the constructions of tests/attention_ref.py, proved in float64 and in plain fp32 torch for exactly the case lists
tests/test_attention_edges_gpu.py runs (imported from attention_ref, not copied)."""
import numpy as np
import pytest
import torch

import attention_ref as A


def test_selector_scale_times_log2e_is_a_power_of_two_in_fp32():
    s = np.float32(A.SELECTOR_SCALE)
    assert float(s) == A.SELECTOR_SCALE, "SELECTOR_SCALE is an fp32 number: a c_float argument carries it unchanged"
    assert np.float32(s * A.LOG2E_F32) == np.float32(A.SELECTOR_C) == np.float32(0.25)
    assert abs(A.SELECTOR_SCALE - np.log(2.0) / 4) < 1e-7


def _bf16x3_exact(x):
    hi = x.bfloat16().float()
    mid = (x - hi).bfloat16().float()
    lo = (x - hi - mid).bfloat16().float()
    return torch.equal(hi + mid + lo, x)


def _f16x2_exact(x, exp):
    s = x * 2.0 ** exp
    hi = s.half().float()
    lo = (s - hi).half().float()
    return bool(torch.isfinite(hi).all()) and torch.equal(hi + lo, s)


@pytest.mark.parametrize("n,tokens,heads,kind", A.SELECTOR_CASES)
def test_selector_inputs(n, tokens, heads, kind):
    qkv, pi, expected = A.selector_qkv(n, tokens, heads, kind)
    C = heads * 32
    assert qkv.shape == (n * tokens, 3 * C) and qkv.dtype == torch.float32 and expected.shape == (n * tokens, C)
    q, k, v = A.heads_of(qkv, n, tokens, heads)
    # the selection: pi is in range, and what the kinds promise
    assert int(pi.min()) >= 0 and int(pi.max()) < tokens
    if kind == "first":
        assert int(pi.max()) == 0
    if kind == "last":
        assert int(pi.min()) == tokens - 1
    if kind == "mix" and tokens > 1:
        assert len({tuple(pi[b, h].tolist()) for b in range(n) for h in range(heads)}) == n * heads, "one map per (sample, head)"
    # float64: the selected key leads by >= 160 binary orders (every other probability is 0 in fp32, denormals included: 2^-149 is the
    # smallest), and every log2-domain score is an integer
    if tokens > 1:
        assert A.log2_lead(qkv, pi, n, tokens, heads) >= 160.0
    s2 = q.double() @ k.double().transpose(-1, -2) * A.SELECTOR_C
    assert torch.equal(s2, s2.round())
    # the F16X2 range: |K|, |V| and the pre-scaled |Q| below 1000
    assert float(k.abs().max()) < 1000.0 and float(v.abs().max()) < 1000.0 and float((q * A.SELECTOR_C).abs().max()) < 1000.0
    # every operand is exact in the three-way bf16 split and in the fp16 hi / lo split of 2^6 x (the probabilities 1 and 0 too: 2^14 x)
    for t in (k, v, q * A.SELECTOR_C):
        assert _bf16x3_exact(t) and _f16x2_exact(t, 6)
    assert _f16x2_exact(torch.tensor([0.0, 1.0]), 14)
    # expected[i] = V[pi(i)], and V tells keys, heads and samples apart
    for b in range(n):
        for h in range(heads):
            assert torch.equal(expected.view(n, tokens, heads, 32)[b, :, h], v[b, h][pi[b, h]])
            assert len({tuple(r.tolist()) for r in v[b, h]}) == tokens, "no two keys share a V row"
    assert len({tuple(v[b, h, 0].tolist()) for b in range(n) for h in range(heads)}) == n * heads
    # float64 (whose other probabilities are tiny, not 0) agrees to 2^-160; plain fp32 torch reproduces it exactly
    out64, _ = A.attention(qkv, n, tokens, heads, A.SELECTOR_SCALE)
    assert float((out64 - expected.double()).abs().max()) <= 2.0 ** -160 * 16 * tokens
    q32, k32, v32 = A.heads_of(qkv, n, tokens, heads)
    out32 = (torch.softmax(q32 @ k32.transpose(-1, -2) * A.SELECTOR_SCALE, -1) @ v32).permute(0, 2, 1, 3).reshape(n * tokens, C)
    assert torch.equal(out32, expected)


@pytest.mark.parametrize("tokens", [2, 1000, 2049, 4096])
def test_selector_holds_at_other_token_counts(tokens):
    """the construction itself, away from the GPU list: 1 head, every kind"""
    for kind in A.KINDS:
        qkv, pi, expected = A.selector_qkv(1, tokens, 1, kind)
        assert A.log2_lead(qkv, pi, 1, tokens, 1) >= 160.0
        q, k, v = A.heads_of(qkv, 1, tokens, 1)
        out32 = (torch.softmax(q @ k.transpose(-1, -2) * A.SELECTOR_SCALE, -1) @ v)[0, 0]
        assert torch.equal(out32, expected)


@pytest.mark.parametrize("n,tokens,heads", A.UNIFORM_CASES)
def test_uniform_inputs(n, tokens, heads):
    qkv, expected = A.uniform_qkv(n, tokens, heads)
    q, k, v = A.heads_of(qkv, n, tokens, heads)
    assert not q.any() and bool(torch.isfinite(k).all()) and float(k.abs().max()) < 1000.0
    assert torch.equal(v, v.round()) and float(v.abs().max()) <= 8.0
    # the sum over the keys is an integer below 2^24: exact in fp32 in any order
    tot = v.double().sum(2)
    assert torch.equal(v.sum(2).double(), tot) and float(tot.abs().max()) < 2 ** 24 and tokens * 8 < 2 ** 24
    out64, _ = A.attention(qkv, n, tokens, heads, 32 ** -0.5)
    assert float((out64 - expected).abs().max()) <= 2.0 ** -44 * 8.0        # (torch rounds every p v product: relative to max |V|)
    # plain fp32 in the order of a flash kernel (normalise last): every probability is exp(0) = 1, l = tokens, the sum exact, and
    # one reciprocal and one product put the result within 2^-22 of the reference, element by element
    s = q @ k.transpose(-1, -2) * 32 ** -0.5
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    assert not s.any() and torch.equal(p, torch.ones_like(p))
    l = p.sum(-1, keepdim=True)
    assert torch.equal(l, torch.full_like(l, tokens)) and torch.equal((p @ v).double(), tot[:, :, None].expand(-1, -1, tokens, -1))
    out32 = ((p @ v) * (1.0 / l)).permute(0, 2, 1, 3).reshape(n * tokens, heads * 32)
    assert bool(((out32.double() - expected).abs() <= 2.0 ** -22 * expected.abs()).all())
    # (torch.softmax normalises FIRST: a rounded 1 / tokens, `tokens` rounded products and as many rounded additions per element, each
    #  an error of up to 2^-24 x 8 / tokens x tokens -- only an absolute bound holds for it)
    soft32, _ = A.attention(qkv, n, tokens, heads, 32 ** -0.5, dtype=torch.float32)
    assert float((soft32.double() - expected).abs().max()) <= tokens * 2.0 ** -23 * 8.0
    # a key counted past the end, or a live key dropped, moves some element by far more than the bound
    vv = v.double()
    dropped = ((tot[:, :, None] - vv) / (tokens - 1)).permute(0, 2, 1, 3).reshape(n * tokens, heads * 32)
    moved = (dropped - expected).abs().max(1).values
    assert float(moved.min()) > 2.0 ** -12 * float(expected.abs().max())


def test_case_lists():
    assert set(A.RAGGED) <= set(A.TOKENS) and (1, 2048, 1) in A.SHAPES and len(A.SHAPES) == 2 * len(A.TOKENS) + 1
    assert {t for _, t, _, _ in A.SELECTOR_CASES} == {1, 33, 65, 129, 257} and {k for *_, k in A.SELECTOR_CASES} == set(A.KINDS)
    assert all((n, h) == (2, 3) for n, _, h, _ in A.SELECTOR_CASES) and all((n, h) == (2, 3) for n, _, h in A.UNIFORM_CASES)
    assert {t for _, t, _ in A.UNIFORM_CASES} == {31, 33, 63, 65, 127, 129, 255, 257}
    assert A.FRONT_ROWS >= 256 + 64 and A.BACK_ROWS >= 256


def test_framing_helpers():
    x = torch.arange(24, dtype=torch.float32).reshape(4, 6)
    alloc, view = A.framed(x, A.NAN, 3, 2)
    assert alloc.shape == (9, 6) and torch.equal(view, x) and view.data_ptr() == alloc.data_ptr() + 3 * 6 * 4
    assert bool(torch.isnan(alloc[:3]).all()) and bool(torch.isnan(alloc[7:]).all())
    assert A.frame_intact(alloc, view, A.NAN)
    view[1, 2] = A.NAN                                  # the middle may change
    assert A.frame_intact(alloc, view, A.NAN)
    alloc[8, 5] = 0.0
    assert not A.frame_intact(alloc, view, A.NAN)
    alloc[8, 5] = -A.NAN                                # another NaN bit pattern is a change too
    assert not A.frame_intact(alloc, view, A.NAN)
    alloc, view = A.framed(x, A.SENT, 2, 2)
    assert A.frame_intact(alloc, view, A.SENT)
    alloc[1, 0] = np.nextafter(np.float32(A.SENT), np.float32(0)).item()
    assert not A.frame_intact(alloc, view, A.SENT)
    # a row fill, several blocks
    fill = A.inf_kv_fill(1)
    blocks = [torch.zeros(5, 96), torch.ones(5, 96)]
    alloc, views = A.framed_blocks(blocks, fill, 4, 3, 2)
    assert alloc.shape == (4 + 5 + 3 + 5 + 2, 96) and torch.equal(views[1], blocks[1])
    assert bool(torch.isnan(alloc[0, :32]).all()) and bool(torch.isinf(alloc[10, 32:]).all())
    assert views[1].data_ptr() - views[0].data_ptr() == (5 + 3) * 96 * 4
    assert A.frame_intact(alloc, views, fill)
    alloc[10, 40] = 1.0                                 # between the blocks
    assert not A.frame_intact(alloc, views, fill)
    # one dimension (the log-sum-exp) and integers (the range flag)
    alloc, view = A.framed(torch.zeros(7), A.SENT, 2, 2)
    assert alloc.shape == (11,) and A.frame_intact(alloc, view, A.SENT)
    alloc[0] = 0.0
    assert not A.frame_intact(alloc, view, A.SENT)
    alloc, view = A.framed(torch.zeros(1, dtype=torch.int32), -7, 4, 4)
    view[0] = 1
    assert A.frame_intact(alloc, view, -7)
    alloc[5] = 0
    assert not A.frame_intact(alloc, view, -7)
    # byte buffers
    alloc, view = A.framed_bytes(100, 0xFF, 64, 32)
    assert alloc.numel() == 196 and bool((view == 0xFF).all()) and alloc.dtype == torch.uint8
    assert torch.equal(alloc[:64], A.byte_pattern(196)[:64]) and len(set(alloc[:64].tolist())) > 32
    view[:] = 3
    assert A.frame_intact(alloc, view, "pattern")
    alloc[164] ^= 1
    assert not A.frame_intact(alloc, view, "pattern")


def test_slabs_sum_in_slab_order():
    qkv, _, _ = A.selector_qkv(2, 33, 3, "mix")
    for nslab in (1, 2, 3):
        slabs, eff = A.split_slabs(qkv, nslab)
        assert len(slabs) == nslab and torch.equal(eff, qkv), "integers: the slabs sum back exactly"
    uq, _ = A.uniform_qkv(2, 33, 3)
    slabs, eff = A.split_slabs(uq, 3)
    C = 96
    assert torch.equal(eff[:, :C], uq[:, :C]) and torch.equal(eff[:, 2 * C:], uq[:, 2 * C:]), "Q = 0 and the integer V survive the slabs"
    got = slabs[0]
    for s in slabs[1:]:
        got = got + s
    assert torch.equal(got, eff)
