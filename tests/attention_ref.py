"""Pure-torch side of the self-attention forward edge tests (tests/test_attention_edges_gpu.py; proved on the CPU by
tests/test_attention_ref_cpu.py): guard-memory framing, the exact "selector" and "uniform" inputs, and the case lists both files use.

Framing.  framed(x, fill, rows_before, rows_after) puts x into the middle of ONE allocation whose other rows hold `fill`;
frame_intact compares every frame element with the fill bit for bit.  Input frames are NaN rows -- the front one at least a
256-query workgroup plus a 64-key tile of [q | k | v] rows deep, the back one a 256-query workgroup -- so that a row read before
sample 0 or behind the last sample lands in ALLOCATED memory and shows as a NaN (or, with inf_kv_fill, as an inf that a zero
probability turns into a NaN), never as a fault.  Output frames hold a sentinel, byte buffers a position-dependent byte pattern.

Selector inputs.  Key j of every (sample, head) is 16 x a +-1 code of j (twelve binary digits of j, each in two columns, the last
eight columns +1), query i is 32 x the code of pi(i): the score of key pi(i) is 32 x 512 x c, that of a key differing in b digits
4 b x 512 x c less, c = scale log2(e).  SELECTOR_SCALE is the fp32 number whose fp32 product with the kernels' fp32 log2(e) is
exactly 2^-2: every log2-domain score is then an INTEGER (a multiple of 128), the selected key leads by >= 512 binary orders, its
probability is exp2(0) = 1 and every other one exp2(<= -512) = 0 in fp32, denormals included.  Integer scores matter for one
kernel: the F16X2 kernel keeps its running maximum on the integer grid (m = ceil(max), csrc/attention_bf16.hip h2_softmax), so a
fractional maximum would give the selected key the probability 2^(max - m) < 1 and leave the quotient to the final normalisation;
on integer scores m is the maximum itself and V[pi(i)] must come out bit for bit from every kernel.  V holds integers in [-8, 8]:
columns 0..11 carry the binary digits of the key with a magnitude that depends on head and sample, the others a residue of
(key, column, head, sample).

Uniform inputs.  Q = 0: every score is 0, every probability equal, the result sum_j V[j] / tokens with an integer sum."""
import math

import numpy as np
import torch

NAN = float("nan")
INF = float("inf")
SENT = -7777.25                       # output sentinel (exact in fp32; no result of these tests comes near it)
QUERY_WORKGROUP = 256                 # the largest query tile of a workgroup (two 32-query blocks per wave, four waves)
KEY_TILE = 64                         # keys per staged / pre-split tile
FRONT_ROWS = QUERY_WORKGROUP + KEY_TILE
BACK_ROWS = QUERY_WORKGROUP
BYTE_FRAME = 4096                     # bytes before and after a framed byte buffer (keeps the 1-KiB alignment of the tile planes)

KINDS = ("first", "last", "reverse", "mix")
TOKENS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
BATCH_HEADS = ((1, 1), (2, 3))
SHAPES = [(n, t, h) for t in TOKENS for n, h in BATCH_HEADS] + [(1, 2048, 1)]
RAGGED = (33, 65, 129)                                                         # batch independence
SELECTOR_CASES = [(2, t, 3, kind) for t in (1, 33, 65, 129, 257) for kind in KINDS]
UNIFORM_CASES = [(2, t, 3) for t in (31, 33, 63, 65, 127, 129, 255, 257)]

K_MAG, Q_MAG = 16.0, 32.0
CODE_BITS = 12                        # keys below 4096
LOG2E_F32 = np.float32(1.4426950408889634)          # the constant of the kernels (scale * LOG2E in fp32)


def _selector_scale():
    """the fp32 scale with fl32(scale * fl32(log2 e)) == 0.25 (one exists: the product moves by 0.72 ulp of 0.25 per ulp of scale)"""
    s = np.float32(0.25 / float(LOG2E_F32))
    for _ in range(8):
        for cand in (s, np.nextafter(s, np.float32(0)), np.nextafter(s, np.float32(1))):
            if np.float32(cand * LOG2E_F32) == np.float32(0.25):
                return float(cand)
        s = np.nextafter(s, np.float32(1))
    raise AssertionError("no fp32 scale gives scale * log2(e) == 0.25")


SELECTOR_SCALE = _selector_scale()
SELECTOR_C = 0.25                     # SELECTOR_SCALE * log2(e), as the kernels form it


# ------------------------------------------------------------------------------------------------------------------- framing
def _rows_fill(shape, fill, dtype, device):
    """a tensor of `shape` whose every row is `fill` (a number or one row)"""
    if torch.is_tensor(fill):
        return fill.to(device=device, dtype=dtype).expand(shape).contiguous()
    return torch.full(shape, fill, dtype=dtype, device=device)


def framed_blocks(blocks, fill, rows_before, rows_between, rows_after, device=None):
    """The blocks (equal shapes [rows, ...]) in ONE allocation: rows_before fill rows, block 0, rows_between fill rows, block 1,
    ..., rows_after fill rows.  Returns (allocation, [views of the blocks])."""
    device = blocks[0].device if device is None else device
    r, rest = blocks[0].shape[0], tuple(blocks[0].shape[1:])
    total = rows_before + len(blocks) * r + (len(blocks) - 1) * rows_between + rows_after
    alloc = _rows_fill((total,) + rest, fill, blocks[0].dtype, device)
    views = []
    for i, b in enumerate(blocks):
        assert tuple(b.shape) == (r,) + rest
        s = rows_before + i * (r + rows_between)
        alloc[s:s + r].copy_(b)
        views.append(alloc[s:s + r])
    return alloc, views


def framed(x, fill, rows_before, rows_after, device=None):
    """x in the middle of one allocation of `fill` rows: (allocation, view of x)"""
    alloc, views = framed_blocks([x], fill, rows_before, 0, rows_after, device)
    return alloc, views[0]


def byte_pattern(nbytes, device="cpu"):
    """the fixed frame pattern of byte buffers: byte i = 131 i + 17 (mod 256)"""
    return ((torch.arange(nbytes, dtype=torch.int64, device=device) * 131 + 17) & 0xFF).to(torch.uint8)


def framed_bytes(nbytes, inner, before=BYTE_FRAME, after=BYTE_FRAME, device="cpu"):
    """`nbytes` bytes of value `inner` between `before` and `after` bytes of byte_pattern: (allocation, view)"""
    alloc = byte_pattern(before + nbytes + after, device)
    alloc[before:before + nbytes] = inner
    return alloc, alloc[before:before + nbytes]


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()])


def frame_intact(alloc, views, fill):
    """every element of `alloc` outside `views` (a view or a list of views, as framed / framed_blocks / framed_bytes returned
    them) still holds its fill, bit for bit (NaN payloads and the sign of zero included).  fill: a number, one row, or
    "pattern" for byte buffers."""
    views = [views] if torch.is_tensor(views) else list(views)
    want = byte_pattern(alloc.numel(), alloc.device) if isinstance(fill, str) else _rows_fill(alloc.shape, fill, alloc.dtype, alloc.device)
    row = alloc[0].numel() if alloc.dim() > 1 else 1
    frame = torch.ones(alloc.shape[0], dtype=torch.bool, device=alloc.device)
    for v in views:
        off = v.storage_offset() - alloc.storage_offset()
        assert off % row == 0 and v.is_contiguous()
        frame[off // row: off // row + v.shape[0]] = False
    return bool((_bits(alloc)[frame] == _bits(want)[frame]).all())


def inf_kv_fill(heads):
    """one [q | k | v] frame row of the zero-probability test: q columns NaN, k and v columns +inf"""
    C = heads * 32
    return torch.cat([torch.full((C,), NAN), torch.full((2 * C,), INF)])


# ---------------------------------------------------------------------------------------------------------------- selector inputs
def code(j):
    """+-1 code of the keys j (int64 tensor [...]) -> [..., 32]: digit b of j in columns 2 b and 2 b + 1 (+1 for a 0 digit), columns 24..31 = +1"""
    bits = (j[..., None] >> torch.arange(CODE_BITS)) & 1
    return torch.cat([(1 - 2 * bits).repeat_interleave(2, -1), torch.ones(j.shape + (32 - 2 * CODE_BITS,), dtype=torch.int64)], -1).float()


def selected_key(kind, n, tokens, heads):
    """pi: int64 [n, heads, tokens] -- the key query i of (sample, head) selects"""
    i = torch.arange(tokens).expand(n, heads, tokens)
    if kind == "first":
        return torch.zeros_like(i)
    if kind == "last":
        return torch.full_like(i, tokens - 1)
    if kind == "reverse":
        return tokens - 1 - i
    assert kind == "mix"
    b, h = torch.arange(n)[:, None, None], torch.arange(heads)[None, :, None]
    return ((2 * (h + heads * b) + 3) * i + 5 * h + 11 * b + 1) % tokens


def small_int_v(n, tokens, heads):
    """V [n, tokens, heads, 32]: integers in [-8, 8] that differ by key, head and sample"""
    b, j, h, d = torch.meshgrid(torch.arange(n), torch.arange(tokens), torch.arange(heads), torch.arange(32), indexing="ij")
    digit = (2 * ((j >> d.clamp(max=CODE_BITS - 1)) & 1) - 1) * (1 + (h + 3 * b) % 8)
    other = (7 * j + 3 * d + 5 * h + 11 * b) % 17 - 8
    return torch.where(d < CODE_BITS, digit, other).float()


def _rows(q, k, v):
    """[n, tokens, heads, 32] x 3 -> the fused projection's rows [n tokens][3 heads 32] (q | k | v)"""
    n, t, h, _ = q.shape
    return torch.cat([x.reshape(n * t, h * 32) for x in (q, k, v)], 1).contiguous()


def selector_qkv(n, tokens, heads, kind):
    """(qkv fp32 [n tokens][3 heads 32], pi [n, heads, tokens], expected fp32 [n tokens][heads 32]); to be run with SELECTOR_SCALE"""
    assert tokens <= 1 << CODE_BITS
    pi = selected_key(kind, n, tokens, heads)
    k = (K_MAG * code(torch.arange(tokens)))[None, :, None, :].expand(n, tokens, heads, 32)
    q = (Q_MAG * code(pi)).permute(0, 2, 1, 3)                                   # [n, tokens, heads, 32]
    v = small_int_v(n, tokens, heads)
    idx = pi.permute(0, 2, 1)[..., None].expand(n, tokens, heads, 32)            # expected[b, i, h] = v[b, pi[b, h, i], h]
    expected = torch.gather(v, 1, idx).reshape(n * tokens, heads * 32).contiguous()
    return _rows(q, k, v), pi, expected


def uniform_qkv(n, tokens, heads, seed=570):
    """(qkv fp32, expected float64 [n tokens][heads 32]): Q = 0, K random (1.5 x standard normal), V small integers;
    expected = sum_j V[j] / tokens, the sum an integer (exact in fp32)"""
    g = torch.Generator().manual_seed(seed + tokens)
    k = 1.5 * torch.randn(n, tokens, heads, 32, generator=g)
    v = small_int_v(n, tokens, heads)
    mean = v.double().sum(1, keepdim=True) / tokens                              # [n, 1, heads, 32]
    expected = mean.expand(n, tokens, heads, 32).reshape(n * tokens, heads * 32).contiguous()
    return _rows(torch.zeros_like(k), k, v), expected


def heads_of(qkv, n, tokens, heads):
    """q, k, v as [n, heads, tokens, 32] (dtype of qkv)"""
    return [t.reshape(n, tokens, heads, 32).permute(0, 2, 1, 3) for t in qkv.split(heads * 32, dim=1)]


def attention(qkv, n, tokens, heads, scale, dtype=torch.float64):
    """softmax(q k^T scale) v in `dtype`, rows as the kernels write them; also the natural log-sum-exp [n, heads, tokens]"""
    q, k, v = [t.to(dtype) for t in heads_of(qkv, n, tokens, heads)]
    s = q @ k.transpose(-1, -2) * scale
    out = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(n * tokens, heads * 32)
    return out, torch.logsumexp(s, -1)


def split_slabs(qkv, nslab, seed=580):
    """qkv as `nslab` raw split-K slabs: slabs 1.. hold integers in [-3, 3], slab 0 the rest.  Returns (slabs, effective) with
    effective = ((slab 0 + slab 1) + slab 2), the fp32 sum in slab order the kernel forms: exactly qkv wherever qkv holds small
    integers (zeros included), within a rounding of it elsewhere -- references are taken from `effective`."""
    g = torch.Generator().manual_seed(seed)
    rest = [torch.randint(-3, 4, qkv.shape, generator=g).float() for _ in range(nslab - 1)]
    first = qkv.clone()
    for r in rest:
        first = first - r
    eff = first.clone()
    for r in rest:
        eff = eff + r
    return [first] + rest, eff


# ------------------------------------------------------------------------------------------- which (entry, tokens) pairs run
OUT_PS_ROWS = 32                      # out_ps: whole 32-row blocks of the PS layout
TILE_ROWS = 64                        # _tiles: whole 64-key tiles
PIPE_ROWS = 256                       # the pipelined key loop: whole 256-query workgroups
SMALL_NW8_MIN_TOKENS = 512            # ldmk_attn_self_small: eight waves from here, four below


def log2_lead(qkv, pi, n, tokens, heads):
    """float64: the least lead, in binary orders, of the selected key's log2-domain score over any other key's (inf for one key)"""
    q, k, _ = [t.double() for t in heads_of(qkv, n, tokens, heads)]
    s = q @ k.transpose(-1, -2) * SELECTOR_C
    sel = torch.gather(s, -1, pi[..., None])
    others = s.masked_fill(torch.nn.functional.one_hot(pi, tokens).bool(), -math.inf)
    return float((sel - others.max(-1, keepdim=True).values).min())
