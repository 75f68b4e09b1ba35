"""GPU: guard-memory, exact and token-edge tests of the self-attention FORWARD entry points -- ldmk_attn_self (one and two query
tiles per wave) and ldmk_attn_self_lse (csrc/attention.hip), ldmk_attn_self_x3, _x3p, _x3p_ps, _h2, _h2_ps, _h2_tiles
(csrc/attention_bf16.hip; LDMK_ATTN_QB 1 / 2, LDMK_ATTN_PIPE 0 / 1 / 2) and ldmk_attn_self_small with 1, 2 and 3 raw slabs
(csrc/attention_small.hip) -- at 1, 2 and every count around a multiple of 32 up to 257 tokens, one and two samples, plus one
2048-token case for the default two-blocks-per-wave route with its lazy loop and the eight-wave small kernel.

Every launch goes through lib.call with raw pointers into FRAMED buffers (tests/attention_ref.py): the [q | k | v] rows (each
slab of them) between allocated NaN rows -- 320 in front, 256 behind, as deep as the largest query workgroup plus a key tile, so
that an over-read shows and cannot fault --, the result, the log-sum-exp and the range flag between sentinels, the pre-split
K / V scratch EXACTLY ldmk_attn_kv_split(_h2)_bytes long and pre-filled with 0xFF bytes (NaN in bf16 and fp16: the zero padding
of the last key tile must have been written), the PS-layout result exactly ldmk_ps_bytes(_h2) long, both inside a byte pattern.

  1. test_framed_random_values   1.5 x standard normal rows: finite, within the float64 bound the existing test of each kernel
                                 states, every frame intact, range flag 0, out_ps = pack_ps(out), a second call the same bits;
                                 and again with +inf in the K and V columns of the frame rows (a masked score must not meet them).
  2. test_batch_independence     ragged counts: sample 0 of a two-sample call is bit for bit the one-sample call on its rows.
  3. test_selector_is_exact      selector inputs (attention_ref): every query selects one key with probability exactly 1: V[pi(i)]
                                 bit for bit, from every entry and form.
  4. test_uniform_is_a_mean      Q = 0: the mean of the V rows within 2^-22, element by element.

Where an entry refuses a count (out_ps: tokens % 32, _tiles: tokens % 64) the refusal and its message are asserted and the
buffers must be untouched; every (entry, shape) pair runs or is refused, and both counts are asserted."""
import os
import re
from types import SimpleNamespace
from typing import NamedTuple

import pytest
import torch

import attention_ref as A
from conftest import rnd
from test_f16x2_gpu import _f16x2_class
from test_ops_gpu import close, ops  # noqa: F401  (the `ops` fixture)
from test_split_gpu import _err, _same_class
from test_switch_arms_gpu import arm  # noqa: F401  (the `arm` fixture)

pytestmark = pytest.mark.gpu

ISENT = -7                                # sentinel around the range flag
SCALE = 32 ** -0.5


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_error():
    """A sticky HIP error (an illegal access is one) ends the session: nothing more is launched on a device that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error during this test, nothing more is launched: {e}", returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _return_the_poisoned_memory():
    """Every buffer of this module ends up filled with NaN, inf, sentinels or 0xFF bytes.  Freed, they would stay in torch's caching
    allocator and be handed to the `torch.empty` of whatever module runs next: give them back to the driver instead, so that the
    modules after this one start from the allocator state they had before this one existed."""
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


class Entry(NamedTuple):
    name: str
    family: str               # "f32" | "x3" | "h2" | "small": whose float64 bound applies
    qt: int = 0               # ldmk_attn_force_qt
    lse: bool = False
    presplit: bool = False    # reads LDMK_ATTN_QB; kv_scratch
    ps: bool = False          # writes out_ps
    out: bool = True          # writes the fp32 result
    tiles: bool = False
    nslab: int = 0


ENTRIES = [Entry("self_qt1", "f32", qt=1), Entry("self_qt2", "f32", qt=2), Entry("self_lse", "f32", lse=True),
           Entry("x3", "x3"), Entry("x3p", "x3", presplit=True), Entry("x3p_ps", "x3", presplit=True, ps=True),
           Entry("h2", "h2", presplit=True), Entry("h2_ps", "h2", presplit=True, ps=True),
           Entry("h2_ps_only", "h2", presplit=True, ps=True, out=False), Entry("h2_tiles", "h2", presplit=True, ps=True, tiles=True),
           Entry("small1", "small", nslab=1), Entry("small2", "small", nslab=2), Entry("small3", "small", nslab=3)]


def refusal(e, tokens):
    """the message with which the entry refuses this count, or None (the REQUIREs of csrc/attention_bf16.hip)"""
    if e.tiles and tokens % A.TILE_ROWS:
        return f"ldmk_attn_self_h2_tiles: tokens={tokens} must be a multiple of 64 (whole K / V tiles)"
    if e.ps and tokens % A.OUT_PS_ROWS:
        return f"ldmk_attn_self_{'h2' if e.family == 'h2' else 'x3p'}_ps: out_ps needs tokens % 32 == 0 ({tokens})"
    return None


def forms(e, tokens, pipes=None):
    """(LDMK_ATTN_QB, LDMK_ATTN_PIPE) pairs an entry is run under (None: the default).  The pre-split kernels: default, one and two
    query blocks per wave; the F16X2 ones with two blocks also every key-loop form in `pipes` (default: 0, 1, 2 where the count is a
    multiple of 256 -- elsewhere no arm pipelines)."""
    if not e.presplit:
        return [(None, None)]
    f = [(None, None), (1, None), (2, None)]
    if e.family == "h2":
        if pipes is None:
            pipes = (0, 1, 2) if tokens % A.PIPE_ROWS == 0 else ()
        f += [(2, p) for p in pipes]
    return f


def expected_counts(tokens):
    """(launched, refused) (entry, form) pairs of one shape in test 1, counted on its own: 3 fp32 entries, x3, 3 small; x3p under 3
    forms, x3p_ps too where tokens % 32 == 0; the four F16X2 entries under 3 forms (6 at a multiple of 256): _h2 always, the two
    _h2_ps where tokens % 32 == 0, _tiles where tokens % 64 == 0; the others are refused once each"""
    h2f = 6 if tokens % 256 == 0 else 3
    ps, tl = tokens % 32 == 0, tokens % 64 == 0
    return 3 + 1 + 3 + 3 + (3 if ps else 0) + h2f * (1 + (2 if ps else 0) + (1 if tl else 0)), (0 if ps else 3) + (0 if tl else 1)


class Bufs:
    """the framed device buffers of one entry on one input"""

    def __init__(self, c, e, slabs, fill):
        so, n, tokens, heads = c.so, c.n, c.tokens, c.heads
        rows, C = n * tokens, heads * 32
        self.e, self.fill = e, fill
        gap = A.FRONT_ROWS + A.BACK_ROWS
        self.qalloc, self.q = A.framed_blocks(slabs, fill, A.FRONT_ROWS, gap, A.BACK_ROWS, device="cuda")
        self.slab_stride = (rows + gap) * 3 * C
        assert len(slabs) < 2 or (self.q[1].data_ptr() - self.q[0].data_ptr() == 4 * self.slab_stride and self.slab_stride > rows * 3 * C)
        self.oalloc, self.out = A.framed(torch.full((rows, C), A.NAN), A.SENT, A.FRONT_ROWS, A.BACK_ROWS, "cuda") if e.out else (None, None)
        self.lalloc, self.lse = A.framed(torch.full((n * heads * tokens,), A.NAN), A.SENT, 64, 64, "cuda") if e.lse else (None, None)
        self.kalloc = self.kv = self.palloc = self.ps = None
        if e.presplit:
            nb = (so.ldmk_attn_kv_split_h2_bytes if e.family == "h2" else so.ldmk_attn_kv_split_bytes)(n, tokens, heads)
            assert nb == n * heads * -(-tokens // 64) * (16384 if e.family == "h2" else 24576)
            self.kalloc, self.kv = A.framed_bytes(nb, 0xFF, device="cuda")
        if e.ps:
            nb = (so.ldmk_ps_bytes_h2 if e.family == "h2" else so.ldmk_ps_bytes)(rows, C)
            assert nb == -(-rows // 32) * (C // 16) * (2048 if e.family == "h2" else 3072)
            self.palloc, self.ps = A.framed_bytes(nb, 0xFF, device="cuda")
        self.falloc, self.flag = A.framed(torch.zeros(1, dtype=torch.int32), ISENT, 16, 16, "cuda")

    def reset(self):
        for t, v in ((self.out, A.NAN), (self.lse, A.NAN), (self.kv, 0xFF), (self.ps, 0xFF), (self.flag, 0)):
            if t is not None:
                t.fill_(v)

    def untouched(self):
        """as reset() left them (after a refused call)"""
        ok = all(bool(torch.isnan(t).all()) for t in (self.out, self.lse) if t is not None)
        return ok and all(bool((t == 0xFF).all()) for t in (self.kv, self.ps) if t is not None) and int(self.flag.item()) == 0

    def assert_frames(self, what):
        for name, alloc, view, fill in (("qkv", self.qalloc, self.q, self.fill), ("out", self.oalloc, self.out, A.SENT),
                                        ("lse", self.lalloc, self.lse, A.SENT), ("kv_scratch", self.kalloc, self.kv, "pattern"),
                                        ("out_ps", self.palloc, self.ps, "pattern"), ("range_flag", self.falloc, self.flag, ISENT)):
            if alloc is not None:
                assert A.frame_intact(alloc, view, fill), f"{what}: the frame around {name} was written"

    def results(self):
        """copies of what the call wrote: name -> tensor"""
        return {k: t.clone() for k, t in (("out", self.out), ("lse", self.lse), ("ps", self.ps)) if t is not None}


def _ptr(t):
    return None if t is None else t.data_ptr()


def launch(c, b, scale):
    """one call of the entry on its framed buffers (no synchronisation)"""
    e, L, st = b.e, c.L, c.ops.stream()
    q, o, dims = _ptr(b.q[0]), _ptr(b.out), (c.n, c.tokens, c.heads, scale, st)
    if e.family == "f32":
        c.so.ldmk_attn_force_qt(e.qt)
        try:
            L.call("ldmk_attn_self_lse", q, o, _ptr(b.lse), *dims) if e.lse else L.call("ldmk_attn_self", q, o, *dims)
        finally:
            c.so.ldmk_attn_force_qt(0)
    elif e.name == "x3":
        L.call("ldmk_attn_self_x3", q, o, *dims)
    elif e.name == "x3p":
        L.call("ldmk_attn_self_x3p", q, _ptr(b.kv), o, *dims)
    elif e.name == "x3p_ps":
        L.call("ldmk_attn_self_x3p_ps", q, _ptr(b.kv), o, _ptr(b.ps), *dims)
    elif e.name == "h2":
        L.call("ldmk_attn_self_h2", q, _ptr(b.kv), o, _ptr(b.flag), *dims)
    elif e.name in ("h2_ps", "h2_ps_only"):
        L.call("ldmk_attn_self_h2_ps", q, _ptr(b.kv), o, _ptr(b.ps), _ptr(b.flag), *dims)
    elif e.name == "h2_tiles":
        if refusal(e, c.tokens) is None:          # the tiles ldmk_attn_self_h2's pre-pass writes (what the fused QKV projection writes)
            L.call("ldmk_attn_self_h2", q, _ptr(b.kv), _ptr(torch.empty(c.n * c.tokens, c.heads * 32, device="cuda")), _ptr(b.flag), *dims)
        L.call("ldmk_attn_self_h2_tiles", q, _ptr(b.kv), o, _ptr(b.ps), _ptr(b.flag), *dims)
    else:
        assert e.family == "small"
        L.call("ldmk_attn_self_small", q, e.nslab, b.slab_stride, o, *dims)


def run(c, b, form, scale=SCALE):
    """reset the buffers, launch under the (LDMK_ATTN_QB, LDMK_ATTN_PIPE) form, synchronise"""
    qb, pipe = form
    b.reset()
    with c.arm("LDMK_ATTN_PIPE", pipe), c.arm("LDMK_ATTN_QB", qb):
        launch(c, b, scale)
    torch.cuda.synchronize()


def context(ops, arm, n, tokens, heads):       # noqa: F811
    from dsml_thesis_amd import lib as L
    return SimpleNamespace(ops=ops, arm=arm, L=L, so=L.load(), n=n, tokens=tokens, heads=heads)


def slabs_of(e, qkv):
    """(the entry's input slabs, the qkv they sum to in the kernel's order)"""
    return A.split_slabs(qkv, e.nslab) if e.nslab > 1 else ([qkv], qkv)


def packed(c, e, out):
    """pack_ps of an fp32 result in the entry's arithmetic (bytes)"""
    if e.family == "h2":
        flag = torch.zeros(1, device="cuda", dtype=torch.int32)
        ps = c.ops.pack_ps(out.contiguous(), h2_flag=flag)
        assert int(flag.item()) == 0
        return ps[0]
    return c.ops.pack_ps(out.contiguous())[0]


def fp32_sibling(c, b, form, scale=SCALE):
    """ldmk_attn_self_h2_ps WITH the fp32 result on the same rows and form, in plain buffers: what the PS-only call must have packed"""
    out, flag = torch.empty(c.n * c.tokens, c.heads * 32, device="cuda"), torch.zeros(1, device="cuda", dtype=torch.int32)
    kv, ps = torch.empty_like(b.kv), torch.empty_like(b.ps)
    with c.arm("LDMK_ATTN_PIPE", form[1]), c.arm("LDMK_ATTN_QB", form[0]):
        c.L.call("ldmk_attn_self_h2_ps", _ptr(b.q[0]), _ptr(kv), _ptr(out), _ptr(ps), _ptr(flag), c.n, c.tokens, c.heads, scale, c.ops.stream())
    torch.cuda.synchronize()
    return out


def fp32_result(c, b, form, scale=SCALE):
    """the entry's fp32 result (the PS-only entry: its sibling's, after the bytes were compared)"""
    if b.out is not None:
        return b.out
    sib = fp32_sibling(c, b, form, scale)
    assert torch.equal(b.ps, packed(c, b.e, sib)), f"{b.e.name} {form}: out_ps is not pack_ps of the fp32 result of the same launch with `out`"
    return sib


def assert_refused(c, b, msg):
    b.reset()
    with pytest.raises(c.L.LdmkError) as err:
        launch(c, b, SCALE)
    assert msg in str(err.value), (msg, str(err.value))
    torch.cuda.synchronize()
    assert b.untouched(), f"{b.e.name}: a refused call wrote to its buffers"
    b.assert_frames(f"{b.e.name} (refused)")


# ---------------------------------------------------------------------------------------------------------------------------------
MAXIMA = {}          # entry -> [max |error|, share of the element-wise bound, share of the class bound (max), (rms)] over all cases


def _record(name, y, ref, rtol, atol, e32=None, err=None, floor=None, rms_factor=None):
    d = (y.detach().cpu().double() - ref).abs()
    row = [float(d.max()), float((d / (atol + rtol * ref.abs())).max()), 0.0, 0.0]
    if e32 is not None:
        row[2:] = [err[0] / max(3.0 * e32[0], floor), err[1] / max(rms_factor * e32[1], 0.3 * floor)]
    old = MAXIMA.setdefault(name, [0.0] * 4)
    MAXIMA[name] = [max(a, b) for a, b in zip(old, row)]
    return row


def held_to_its_bound(e, y, ref, e32, what):
    """the float64 bound of the existing test of each kernel: test_ops_gpu.test_attn_self close(1e-4, 2e-5);
    test_split_gpu.test_split_attention_... / test_f16x2_gpu.test_f16x2_attention_...: the class of the fp32 kernel (floor 2e-6) and
    3e-6 element-wise; test_small_batch_gpu.test_attn_self_small close(1e-4, 1e-4)"""
    assert bool(torch.isfinite(y).all()), f"{what}: the result is not finite"
    if e.family in ("x3", "h2"):
        err = _err(y, ref)
        row = _record(e.name, y, ref, 3e-6, 3e-6, e32, err, 2e-6, 1.5 if e.family == "x3" else 2.0)
        print(f"{what}: max |err| {row[0]:.3e}  element-wise {row[1]:.3f}  class max {row[2]:.3f} rms {row[3]:.3f} of the bound")
        (_same_class if e.family == "x3" else _f16x2_class)(e32, err, 2e-6)
        close(y, ref.float(), 3e-6, 3e-6)
    else:
        tol = (1e-4, 2e-5) if e.family == "f32" else (1e-4, 1e-4)
        row = _record(e.name, y, ref, *tol)
        print(f"{what}: max |err| {row[0]:.3e}  {row[1]:.3f} of the bound")
        close(y, ref.float(), *tol)


def lse_bound(qkv, heads):
    """absolute error bound of a log-sum-exp: that of an fp32 score -- 32 products and as many additions, each rounded, of terms that
    sum to at most |q| |k| scale (Cauchy-Schwarz) -- which the maximum and the logarithm of the sum pass on unamplified; the
    caller adds 2^-21 |ref| for the logarithm and the two final roundings"""
    C = heads * 32
    q, k = qkv[:, :C].reshape(-1, heads, 32).double().norm(dim=-1).max(), qkv[:, C:2 * C].reshape(-1, heads, 32).double().norm(dim=-1).max()
    return 66 * 2.0 ** -24 * float(q * k) * SCALE


@pytest.mark.parametrize("fill", ["nan", "inf"])
@pytest.mark.parametrize("n,tokens,heads", A.SHAPES)
def test_framed_random_values(ops, arm, n, tokens, heads, fill):       # noqa: F811
    """Tests 1 and 5.  fill = "nan": NaN frame rows; "inf": +inf in their K and V columns -- a row of the frame that a kernel reads
    and then masks (score -inf, probability 0) would still give 0 x inf = NaN."""
    c = context(ops, arm, n, tokens, heads)
    qkv = 1.5 * rnd(550, n * tokens, 3 * heads * 32)
    row_fill = A.NAN if fill == "nan" else A.inf_kv_fill(heads)
    refs, e32, ran, refused = {}, None, 0, 0
    for e in ENTRIES:
        slabs, eff = slabs_of(e, qkv)
        if e.nslab not in refs:
            refs[e.nslab] = A.attention(eff, n, tokens, heads, SCALE)
        ref, lse_ref = refs[e.nslab]
        b = Bufs(c, e, slabs, row_fill)
        msg = refusal(e, tokens)
        if msg is not None:
            assert_refused(c, b, msg)
            refused += 1
            continue
        for form in forms(e, tokens):
            what = f"{e.name} QB={form[0]} PIPE={form[1]} ({n}, {tokens}, {heads}) {fill}"
            run(c, b, form)
            b.assert_frames(what)
            assert int(b.flag.item()) == 0, f"{what}: range flag"
            y = fp32_result(c, b, form)
            if e32 is None:
                assert e.name == "self_qt1"
                e32 = _err(y, ref)
            held_to_its_bound(e, y, ref, e32, what)
            if e.lse:
                assert bool(((b.lse.cpu().double() - lse_ref.reshape(-1)).abs() <= lse_bound(qkv, heads) + 2.0 ** -21 * lse_ref.reshape(-1).abs()).all()), what
            if b.ps is not None and b.out is not None:
                assert torch.equal(b.ps, packed(c, e, b.out)), f"{what}: out_ps is not pack_ps of the fp32 result of the same call"
            first = b.results()
            run(c, b, form)
            for k, t in b.results().items():
                assert torch.equal(A._bits(t), A._bits(first[k])), f"{what}: a second call gave other bits in {k}"
            ran += 1
    assert (ran, refused) == expected_counts(tokens)


def test_every_pair_runs_or_is_refused():
    """the totals of test_framed_random_values per frame fill, from the host rules alone; both small-kernel forms are in the list"""
    pairs = [(e, s) for e in ENTRIES for s in A.SHAPES]
    ran = sum(len(forms(e, t)) for e, (_, t, _) in pairs if refusal(e, t) is None)
    refused = sum(1 for e, (_, t, _) in pairs if refusal(e, t) is not None)
    assert (ran, refused) == tuple(map(sum, zip(*(expected_counts(t) for _, t, _ in A.SHAPES)))) == (RAN_TOTAL, REFUSED_TOTAL)
    assert sum(1 for e, (_, t, _) in pairs if refusal(e, t) is None) + refused == len(ENTRIES) * len(A.SHAPES)
    assert any(t >= A.SMALL_NW8_MIN_TOKENS for _, t, _ in A.SHAPES) and any(t < A.SMALL_NW8_MIN_TOKENS for _, t, _ in A.SHAPES)
    src = open(os.path.join(os.path.dirname(__file__), "..", "dsml_thesis_amd", "csrc", "attention_small.hip")).read()
    assert re.search(r"if \(tokens >= %d\) \{\s*if \(nslab > 1\) hipLaunchKernelGGL\(\(attn_small_kernel<8, true>\)" % A.SMALL_NW8_MIN_TOKENS, src), \
        "ldmk_attn_self_small: the rule for eight waves moved -- SMALL_NW8_MIN_TOKENS and the shape list follow it"
    for name, row in sorted(MAXIMA.items()):      # (the figures of profiles/attention_edges_errors.txt: run the file with -s)
        print(f"maxima {name:12s} max |err| {row[0]:.3e}  element-wise {row[1]:.3f}  class max {row[2]:.3f} rms {row[3]:.3f}")


@pytest.mark.parametrize("tokens", A.RAGGED)
def test_batch_independence(ops, arm, tokens):       # noqa: F811
    """Test 2.  Sample 0's last key tile borders sample 1's rows: its results from the two-sample call are the bits of a
    one-sample call on its rows alone (between NaN rows).  Every entry that takes the count (the PS-layout entries refuse ragged
    counts: asserted in test_framed_random_values)."""
    n, heads = 2, 3
    c2, c1 = context(ops, arm, n, tokens, heads), context(ops, arm, 1, tokens, heads)
    qkv = 1.5 * rnd(551, n * tokens, 3 * heads * 32)
    ran = 0
    for e in ENTRIES:
        if refusal(e, tokens) is not None:
            continue
        slabs, _ = slabs_of(e, qkv)
        b2, b1 = Bufs(c2, e, slabs, A.NAN), Bufs(c1, e, [s[:tokens].contiguous() for s in slabs], A.NAN)
        for form in forms(e, tokens):
            run(c2, b2, form)
            run(c1, b1, form)
            assert bool(torch.isfinite(b2.out).all()) and torch.equal(b2.out[:tokens], b1.out), f"{e.name} {form}: sample 0 depends on sample 1"
            if e.lse:
                assert torch.equal(b2.lse[:heads * tokens], b1.lse)
            ran += 1
    assert ran == 3 + 1 + 3 + 3 + 3


SELECTOR_PIPES = (0, 1)


@pytest.mark.parametrize("n,tokens,heads,kind", A.SELECTOR_CASES)
def test_selector_is_exact(ops, arm, n, tokens, heads, kind):       # noqa: F811
    """Test 3.  Every query gives one key the probability exp2(0) = 1 and every other key exp2(<= -512) = 0; l = 1; every
    correction of the running output is exp2(0) or exp2(-huge) = 0; V is exact in both splits: V[pi(i)] bit for bit from every
    entry, every LDMK_ATTN_QB / query-tile / slab form and LDMK_ATTN_PIPE 0 and 1.  The scale argument is
    attention_ref.SELECTOR_SCALE: log2-domain scores are integers, which the F16X2 kernel's integer-grid running maximum needs for a
    probability of exactly 1 (see attention_ref).
    NOT covered here: the lazy-maximum key loop (LDMK_ATTN_PIPE=2 with two blocks per wave at multiples of 256 tokens).  Its
    documented range is a rise of about 92 binary orders of a block over its row's maximum, which cannot coexist with
    probabilities that are exactly zero; it is held by test_framed_random_values (256 and 2048 tokens) and by the existing
    lazy-maximum tests.  (The counts of this test are no multiples of 256: LDMK_ATTN_PIPE 0 and 1 are run because a launcher that
    pipelined a ragged count would show here.)"""
    c = context(ops, arm, n, tokens, heads)
    qkv, _, expected = A.selector_qkv(n, tokens, heads, kind)
    ran = 0
    for e in ENTRIES:
        if refusal(e, tokens) is not None:
            continue
        slabs, eff = slabs_of(e, qkv)
        assert torch.equal(eff, qkv)
        b = Bufs(c, e, slabs, A.NAN)
        for form in forms(e, tokens, SELECTOR_PIPES):
            what = f"{e.name} QB={form[0]} PIPE={form[1]} ({n}, {tokens}, {heads}) {kind}"
            run(c, b, form, A.SELECTOR_SCALE)
            got = b.out.cpu()
            bad = (got != expected).nonzero()
            assert torch.equal(got, expected), (f"{what}: {len(bad)} elements differ from V[pi(i)]; the first at (row, column) {bad[0].tolist()}: "
                                                f"{got[tuple(bad[0])].item()!r} for {expected[tuple(bad[0])].item()!r}")
            assert int(b.flag.item()) == 0, what
            b.assert_frames(what)
            if e.lse:       # exp2(0) alone in the sum: the log-sum-exp is the selected score, 32 x 16 x 32 x SELECTOR_SCALE
                assert float((b.lse.cpu().double() - 16384.0 * A.SELECTOR_SCALE).abs().max()) <= 16384.0 * A.SELECTOR_SCALE * 2.0 ** -22
            ran += 1
    assert ran == 3 + 1 + 3 + 3 + (3 + len(SELECTOR_PIPES))


@pytest.mark.parametrize("n,tokens,heads", A.UNIFORM_CASES)
def test_uniform_is_a_mean(ops, arm, n, tokens, heads):       # noqa: F811
    """Test 4.  Q = 0: every score 0, every probability exp2(0), l = tokens and sum_j V[j] an integer -- both exact; what is left
    is one reciprocal (<= 1 ulp) and one product rounding: |got - ref| <= 2^-22 |ref|, element by element.  A key counted past
    `tokens`, or a live key dropped, moves an element by about 1 / 257 of it or more (test_attention_ref_cpu)."""
    c = context(ops, arm, n, tokens, heads)
    qkv, expected = A.uniform_qkv(n, tokens, heads)
    ran = 0
    for e in ENTRIES:
        if refusal(e, tokens) is not None:
            continue
        slabs, eff = slabs_of(e, qkv)
        C = heads * 32
        assert not eff[:, :C].any() and torch.equal(eff[:, 2 * C:], qkv[:, 2 * C:])
        b = Bufs(c, e, slabs, A.NAN)
        for form in forms(e, tokens):
            what = f"{e.name} QB={form[0]} PIPE={form[1]} ({n}, {tokens}, {heads})"
            run(c, b, form)
            d = (b.out.cpu().double() - expected).abs()
            worst = float((d / expected.abs().clamp(min=2.0 ** -40)).max())
            print(f"{what}: worst |got - ref| / |ref| = {worst * 2 ** 22:.3f} x 2^-22")
            assert bool((d <= 2.0 ** -22 * expected.abs()).all()), f"{what}: {worst * 2 ** 22:.3f} x 2^-22"
            assert int(b.flag.item()) == 0, what
            b.assert_frames(what)
            ran += 1
    assert ran == 3 + 1 + 3 + 3 + 3


RAN_TOTAL, REFUSED_TOTAL = 515, 82        # launched and refused (entry, form) pairs over attention_ref.SHAPES, per frame fill
