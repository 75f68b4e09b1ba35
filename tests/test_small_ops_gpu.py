"""Op-level parity of the small kernels (csrc/small.hip) and the row softmax (csrc/attention.hip) against the same
operation in float64 on the CPU, built from the fp32 inputs, at the shapes where such kernels go wrong: tails that are
no multiple of the tile, leading dimensions wider than the row, both clamps of the step counter, and totals beyond the
1 048 576 elements that one pass of a `grid_for()` launch (256 threads x 4096 workgroups) covers.

Metrics (none wider than what the project already states for the same operation):
  sums        max|got - ref| <= rtol * max|ref|   (`_close` of tests/test_backward_gpu.py), rtol 2e-5
  softmax     assert_close rtol 1e-4 / atol 1e-5  (test_bmm_softmax_postprocess)
  samplers    assert_close rtol 1e-6 / atol 2e-6 (x_prev), 4e-6 (pred_x0)   (test_sampler_updates_golden)
  conv1x1     assert_close rtol 1e-5 / atol 1e-5
  data moves  torch.equal
Every bound was checked on the CPU to hold for a plain fp32 torch evaluation of the same formula at these inputs."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rnd
from oracle import ldm_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GRID_PASS = 256 * 4096            # elements one pass of a grid_for() launch covers


@pytest.fixture(scope="module")
def ops():
    from dsml_thesis_amd import ops as ops_
    from dsml_thesis_amd import lib
    lib.load()
    return ops_


@pytest.fixture(scope="module")
def L():
    from dsml_thesis_amd import lib
    lib.load()
    return lib


def _close(got, ref, rtol, what):
    ref = ref.to(torch.float64)
    err = (got.detach().cpu().to(torch.float64) - ref).abs().max().item()
    bound = rtol * max(ref.abs().max().item(), 1e-30)
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def _assert_close(got, ref, rtol, atol):
    torch.testing.assert_close(got.detach().cpu().double(), ref.double(), rtol=rtol, atol=atol)


def _padded(rows, cols, pad):
    """(wide sentinel-filled CUDA buffer [rows][cols + pad], its [rows][cols] view)"""
    wide = torch.full((rows, cols + pad), SENTINEL, device="cuda", dtype=torch.float32)
    return wide, wide[:, :cols]


# ------------------------------------------------------------------------------------------ dense_small
DS_K = (1, 7, 130, 512, 513, 640, 1030)
DS_N = (4, 60, 64, 68, 1000)
DS_ROWS = {False: (1, 16, 17, 33), True: (1, 2, 3, 4)}


def dense_inputs(K, N, rows):
    """x is a [rows][K] column slice of a [rows][K + 3] tensor (ldx > K); weights in the packed [K][N] layout."""
    seed = 1000 + 7 * K + N
    return rnd(seed, rows, K + 3), rnd(seed + 1, K, N), rnd(seed + 2, N)


def dense_ref(x, w, b, silu, dtype=torch.float64):
    xa = x.to(dtype)
    if silu:
        xa = F.silu(xa)
    y = xa @ w.to(dtype)
    return y if b is None else y + b.to(dtype)


def _dense_case(ops, K, N, form4, rows_set):
    rmax = max(rows_set)
    xw, w, b = dense_inputs(K, N, rmax)
    xd, wd, bd = xw.cuda(), w.cuda(), b.cuda()
    for silu, bias, pad in itertools.product((False, True), (False, True), (False, True)):
        ref = dense_ref(xw[:, :K], w, b if bias else None, silu)
        what = f"dense_small form4={form4} K={K} N={N} silu={silu} bias={bias} pad={pad}"
        x_in = xd[:, :K] if pad else xd[:, :K].contiguous()
        outs = {}
        for rows in rows_set:
            wide, out = _padded(rows, N, 8 if pad else 0)
            ops.dense_small(x_in[:rows], wd, bd if bias else None, silu_in=silu, out=out, form4=form4)
            _close(out, ref[:rows], 2e-5, f"{what} rows={rows}")
            if pad:
                assert torch.all(wide[:, N:] == SENTINEL), f"{what} rows={rows}: wrote into the padding of out"
            outs[rows] = out.clone()
            # a row's result does not depend on how many rows share the launch (include/ldmk.h)
            assert torch.equal(out[:1], outs[rows_set[0]][:1]), f"{what}: row 0 differs between 1 and {rows} rows"
        again = ops.dense_small(x_in, wd, bd if bias else None, silu_in=silu, form4=form4)
        assert torch.equal(again, outs[rmax]), f"{what}: two calls differ"
        if silu and bias:
            for r in range(rmax):
                one = ops.dense_small(x_in[r:r + 1], wd, bd, silu_in=True, form4=form4)
                assert torch.equal(one[0], outs[rmax][r]), f"{what}: row {r} of {rmax} differs from its one-row launch"
            for rows in rows_set:
                assert torch.equal(outs[rows], outs[rmax][:rows]), f"{what}: {rows}-row launch differs from {rmax}-row launch"


@pytest.mark.parametrize("form4", [False, True], ids=["scalar", "b128"])
@pytest.mark.parametrize("K", DS_K)
def test_dense_small_float64(ops, K, form4):
    """ldmk_dense_small, scalar form and 16-byte form (silu_in & 2), against float64 `silu(x) @ w + b`: one and several
    512-deep K tiles with tails that are no multiple of 4, 8 or 16; N below, at and above one 64-column workgroup; SiLU
    on / off; bias / None; ldx > K and ldo > N (padding untouched).  Bound: 2e-5 * max|ref| (K-sums up to ~1k terms).
    Bitwise: two calls agree, and row r of a multi-row launch equals the one-row launch of that row."""
    for N in DS_N:
        _dense_case(ops, K, N, form4, DS_ROWS[form4])


@pytest.mark.parametrize("form4", [False, True], ids=["scalar", "b128"])
def test_dense_small_emb_layers_shape(ops, form4):
    """The 640 x 7040 `emb_layers` matrix (110 workgroups of columns), same reference, bound and bitwise checks."""
    _dense_case(ops, 640, 7040, form4, (1, 4) if form4 else (1, 17))


def test_dense_small_form4_rejections(ops, L):
    """The 16-byte form refuses, before any launch: rows = 5, N % 4 != 0, ldo % 4 != 0, and w, bias or out one float
    off a 16-byte boundary (all buffers are valid memory of the full size)."""
    K, N = 16, 8
    x = torch.zeros(5, K, device="cuda")
    w, b = torch.zeros(K, N, device="cuda"), torch.zeros(N, device="cuda")

    def off1(*shape):
        n = int(np.prod(shape))
        return torch.zeros(n + 1, device="cuda")[1:].view(*shape)

    ops.dense_small(x[:4], w, b, form4=True)                                       # the accepted neighbour of every case below
    with pytest.raises(L.LdmkError, match="16-byte form"):
        ops.dense_small(x, w, b, form4=True)                                       # rows = 5
    with pytest.raises(L.LdmkError, match="16-byte form"):
        ops.dense_small(x[:4], torch.zeros(K, 6, device="cuda"), None, form4=True)       # N = 6
    with pytest.raises(L.LdmkError, match="16-byte form"):
        ops.dense_small(x[:4], w, b, out=torch.zeros(4, N + 2, device="cuda")[:, :N], form4=True)      # ldo = 10
    with pytest.raises(L.LdmkError, match="16-byte form"):
        ops.dense_small(x[:4], off1(K, N), b, form4=True)
    with pytest.raises(L.LdmkError, match="16-byte form"):
        ops.dense_small(x[:4], w, off1(N), form4=True)
    with pytest.raises(L.LdmkError, match="16-byte form"):
        ops.dense_small(x[:4], w, b, out=off1(4, N), form4=True)
    ops.dense_small(x, torch.zeros(K, 6, device="cuda"), None)                      # the scalar form takes all of these
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ timestep embedding
def timestep_inputs(n):
    t = np.concatenate([[999, 0, 1], np.random.RandomState(77).randint(0, 1000, size=max(n - 3, 0))])
    return torch.from_numpy(t[:n].astype(np.int64))


def timestep_ref(t, freqs, dim):
    """float64 cos | sin of the fp32 product float(t) * freqs[i] (the argument the kernel rounds to), zero pad column"""
    arg = (t.to(torch.float32)[:, None] * freqs[None]).double()
    ref = torch.zeros(t.shape[0], dim, dtype=torch.float64)
    half = dim // 2
    ref[:, :half], ref[:, half:2 * half] = torch.cos(arg), torch.sin(arg)
    return ref


@pytest.mark.parametrize("n", [1, 3, 257])
@pytest.mark.parametrize("dim", [2, 160, 161, 320])
def test_timestep_embedding_float64(ops, dim, n):
    """ldmk_timestep_embedding: the kernel rounds float(t) * freqs[i] to fp32, evaluates cos and sin in double and rounds
    once, so against float64 cos / sin of that same fp32 argument |err| <= 2**-23 (half an ulp of a value in [-1, 1] is
    2**-25).  Odd dim: the last column is exactly zero.  t includes 0, 1 and 999 (n = 1 runs each of them)."""
    freqs = ops.timestep_freqs(dim, device="cpu")
    ts = [timestep_inputs(3)[i:i + 1] for i in range(3)] if n == 1 else [timestep_inputs(n)]
    for t in ts:
        wide, out = _padded(t.shape[0], dim, 0)
        ops.timestep_embedding(t.cuda(), freqs.cuda(), dim, out=out)
        got = out.cpu().double()
        err = (got - timestep_ref(t, freqs, dim)).abs().max().item()
        assert err <= 2.0 ** -23, f"dim={dim} n={n}: |err| {err:.3e} > 2^-23"
        if dim & 1:
            assert torch.all(out[:, dim - 1] == 0.0)


# ------------------------------------------------------------------------------------------ conv1x1_nchw
def conv1x1_inputs(n, cin, cout, hw):
    return rnd(300 + hw, n, cin, hw, 1), rnd(301 + hw, cout, cin, 1, 1), rnd(302 + hw, cout)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("n,cin,cout,hw", [(2, 3, 3, 4096), (1, 4, 4, 1000), (3, 8, 4, 257)])
def test_conv1x1_nchw_float64(ops, n, cin, cout, hw, bias):
    """ldmk_conv1x1_nchw against float64 F.conv2d; rtol 1e-5 / atol 1e-5.  Pixel counts at, below and ragged above a
    256-thread workgroup, cin != cout."""
    x, w, b = conv1x1_inputs(n, cin, cout, hw)
    ref = F.conv2d(x.double(), w.double(), b.double() if bias else None)
    got = ops.conv1x1_nchw(x.cuda(), w.cuda(), b.cuda() if bias else None)
    _assert_close(got, ref, 1e-5, 1e-5)


# ------------------------------------------------------------------------------------------ softmax_rows
def softmax_inputs(cols):
    x = rnd(400 + cols, 3, cols) * 3.0
    x[1, (cols * 2) // 3] = x[1].max() + 50.0          # one entry 50 above the rest of its row
    return x


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("cols", [1, 77, 256, 257, 4096, 8192])
def test_softmax_rows_float64(ops, cols, scale):
    """ldmk_softmax_rows (in place, row cached in 32 registers per thread) against float64 softmax(x * scale); rtol 1e-4 /
    atol 1e-5 as in test_bmm_softmax_postprocess.  One column, below / at / above one pass of 256 threads, the full 8192."""
    x = softmax_inputs(cols)
    ref = torch.softmax(x.double() * scale, -1)
    wide = torch.full((3 * cols + 8,), SENTINEL, device="cuda")
    got = wide[:3 * cols].view(3, cols)
    got.copy_(x)
    ops.softmax_rows_(got, scale)
    _assert_close(got, ref, 1e-4, 1e-5)
    assert torch.all(wide[3 * cols:] == SENTINEL)


def test_softmax_rows_rejects_wide_rows(ops, L):
    with pytest.raises(L.LdmkError, match="8192"):
        ops.softmax_rows_(torch.zeros(1, 8193, device="cuda"), 1.0)


# ------------------------------------------------------------------------------------------ sampler updates
@pytest.fixture(scope="module")
def sched():
    from dsml_thesis_amd import schedule as S_
    s = O.register_schedule(**W.SCHEDULE)
    ts = O.make_ddim_timesteps(200)
    ac = s["alphas_cumprod"]
    ac = ac.cpu() if torch.is_tensor(ac) else torch.as_tensor(ac)
    return dict(s=s, ts=ts, inv=torch.from_numpy(S_.ddim_inversion_table(ac, ts)),
                fwd=torch.from_numpy(S_.ddim_step_table(ac, ts, 1.0)))


def ddim_ref(x, e, noise, row, dtype=torch.float64):
    """ddim.py:170-203 from one fp32 table row (a_t, a_prev, sigma, sqrt(1 - a_t))"""
    a_t, a_prev, sigma, s1m = (row[i].to(dtype) for i in range(4))
    x, e = x.to(dtype), e.to(dtype)
    p0 = (x - s1m * e) / a_t.sqrt()
    xp = a_prev.sqrt() * p0 + (1.0 - a_prev - sigma * sigma).sqrt() * e
    if noise is not None:
        xp = xp + sigma * noise.to(dtype)
    return xp, p0


def _ddim_call(L, ops, x, e, noise, table, step, xp, p0, tsd, tsbuf, n_ts, advance, n_steps):
    n = x.shape[0]
    L.call("ldmk_ddim_step", x.data_ptr(), e.data_ptr(), 0 if noise is None else noise.data_ptr(), table.data_ptr(),
           step.data_ptr(), 1.0, 0, xp.data_ptr(), 0 if p0 is None else p0.data_ptr(), x[0].numel(), n,
           0 if tsd is None else tsd.data_ptr(), 0 if tsbuf is None else tsbuf.data_ptr(), n_ts, advance, n_steps, ops.stream())


@pytest.mark.parametrize("start,advance,n_ts,with_p0,with_noise", [
    (0, -1, 1, True, False),          # inversion from index 0 upwards
    (199, -1, 300, False, False),     # inversion at the last index: the counter clamps at n_steps - 1
    (0, +1, 2, True, True),           # sampling at index 0: the counter clamps at 0
    (199, +1, 300, False, True),
])
def test_ddim_step_directions_and_clamps(ops, L, sched, start, advance, n_ts, with_p0, with_noise):
    """ldmk_ddim_step against the float64 update built from the fp32 table row and fp32 inputs; rtol 1e-6, atol 2e-6
    (x_prev) / 4e-6 (pred_x0) as in test_sampler_updates_golden.  advance = -1 uses the inversion table rows
    (a_prev, a_t, 0, sqrt(1 - a_prev)); three calls in a row follow the counter.  pred_x0 = NULL; n_ts in {1, n, 300}
    (the write loop passes its 256 threads) with the words behind ts[n_ts) untouched."""
    n, S = 2, 200
    tab = sched["inv"] if advance < 0 else sched["fwd"]
    table = tab.cuda()
    tsd = torch.from_numpy(sched["ts"].astype(np.int64)).cuda()
    x, e = rnd(31, n, 3, 20, 12), rnd(32, n, 3, 20, 12)
    noise = rnd(33, n, 3, 20, 12) if with_noise else None
    step = torch.tensor([start], dtype=torch.int32, device="cuda")
    tsbuf = torch.full((n_ts + 4,), -5, dtype=torch.int64, device="cuda")
    xd, ed, nd = x.cuda(), e.cuda(), None if noise is None else noise.cuda()
    index = start
    for _ in range(3):
        xp = torch.full_like(xd, SENTINEL)
        p0 = torch.full_like(xd, SENTINEL) if with_p0 else None
        _ddim_call(L, ops, xd, ed, nd, table, step, xp, p0, tsd, tsbuf, n_ts, advance, S)
        rx, rp = ddim_ref(xd.cpu(), e, noise, tab[index])
        _assert_close(xp, rx, 1e-6, 2e-6)
        if with_p0:
            _assert_close(p0, rp, 1e-6, 4e-6)
        index = min(max(index - advance, 0), S - 1)
        assert step.item() == index
        assert tsbuf[:n_ts].tolist() == [int(sched["ts"][index])] * n_ts and tsbuf[n_ts:].tolist() == [-5] * 4
        xd = xp
    assert index == {(0, -1): 3, (199, -1): 199, (0, 1): 0, (199, 1): 196}[(start, advance)]


def test_ddim_step_without_advance_keeps_counter(ops, L, sched):
    """advance = 0: no timesteps / ts arguments, the counter stays (the CFG / extras path of the sampler)."""
    table = sched["fwd"].cuda()
    x, e = rnd(34, 1, 3, 5, 7), rnd(35, 1, 3, 5, 7)
    step = torch.tensor([57], dtype=torch.int32, device="cuda")
    xp = torch.empty(1, 3, 5, 7, device="cuda")
    _ddim_call(L, ops, x.cuda(), e.cuda(), None, table, step, xp, None, None, None, 0, 0, 0)
    _assert_close(xp, ddim_ref(x, e, None, sched["fwd"][57])[0], 1e-6, 2e-6)
    assert step.item() == 57


def sampler_large_inputs():
    n, shape = 3, (4, 300, 300)               # 1 080 000 elements: the grid-stride loop takes a second pass
    return rnd(36, n, *shape), rnd(37, n, *shape), rnd(38, n, *shape)


def test_ddim_step_grid_stride(ops, L, sched):
    """per_sample * n = 1 080 000 > 1 048 576: every element past the first grid pass is written, once; same bounds."""
    x, e, noise = sampler_large_inputs()
    assert x.numel() > GRID_PASS
    table = sched["fwd"].cuda()
    tsd = torch.from_numpy(sched["ts"].astype(np.int64)).cuda()
    step = torch.tensor([120], dtype=torch.int32, device="cuda")
    tsbuf = torch.zeros(3, dtype=torch.int64, device="cuda")
    xd, ed, nd = x.cuda(), e.cuda(), noise.cuda()
    xp, p0 = torch.full_like(xd, SENTINEL), torch.full_like(xd, SENTINEL)
    _ddim_call(L, ops, xd, ed, nd, table, step, xp, p0, tsd, tsbuf, 3, 1, 200)
    rx, rp = ddim_ref(x, e, noise, sched["fwd"][120])
    _assert_close(xp, rx, 1e-6, 2e-6)
    _assert_close(p0, rp, 1e-6, 4e-6)
    assert step.item() == 119 and tsbuf.tolist() == [int(sched["ts"][119])] * 3


def ddpm_ref(x, e, noise, s, t, dtype=torch.float64):
    """ddpm.py:215-228,1049-1109 from the fp32 schedule tables, per-sample t; no noise at t = 0"""
    sh = (-1,) + (1,) * (x.dim() - 1)
    g = lambda k: torch.as_tensor(s[k]).cpu().float()[t].to(dtype).view(sh)
    x, e = x.to(dtype), e.to(dtype)
    x0 = g("sqrt_recip_alphas_cumprod") * x - g("sqrt_recipm1_alphas_cumprod") * e
    mean = g("posterior_mean_coef1") * x0 + g("posterior_mean_coef2") * x
    if noise is None:
        return mean
    nz = (t != 0).to(dtype).view(sh)
    return mean + nz * (0.5 * g("posterior_log_variance_clipped")).exp() * noise.to(dtype)


@pytest.mark.parametrize("with_noise", [True, False])
def test_ddpm_step_grid_stride(ops, L, sched, with_noise):
    """ldmk_ddpm_step at 1 080 000 elements with per-sample t = (0, 700, 999) against the float64 ancestral update from the
    fp32 tables: no noise enters the t = 0 sample; noise = NULL.  rtol 1e-6 / atol 2e-6 as in test_sampler_updates_golden."""
    s = sched["s"]
    x, e, noise = sampler_large_inputs()
    t = torch.tensor([0, 700, 999])
    tables = torch.stack([torch.as_tensor(s[k]).float() for k in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                                                                 "posterior_mean_coef1", "posterior_mean_coef2")], 1).contiguous().cuda()
    logvar = torch.as_tensor(s["posterior_log_variance_clipped"]).float().cuda()
    xd, ed, nd, td = x.cuda(), e.cuda(), noise.cuda() if with_noise else None, t.cuda()
    xp = torch.full_like(xd, SENTINEL)
    L.call("ldmk_ddpm_step", xd.data_ptr(), ed.data_ptr(), 0 if nd is None else nd.data_ptr(), tables.data_ptr(), logvar.data_ptr(),
           td.data_ptr(), xp.data_ptr(), x[0].numel(), 3, ops.stream())
    _assert_close(xp, ddpm_ref(x, e, noise if with_noise else None, s, t), 1e-6, 2e-6)


@pytest.mark.parametrize("start,advance,expect", [(5, 1, 4), (5, -1, 6), (0, 1, 0), (19, -1, 19), (1, 1, 0), (18, -1, 19)])
@pytest.mark.parametrize("n_ts", [1, 300])
def test_advance_timestep(ops, L, start, advance, expect, n_ts):
    """ldmk_advance_timestep on its own: +1 walks down, -1 up, both clamp at the ends of the table; ts[0, n_ts) <-
    timesteps[new index], nothing behind it."""
    S = 20
    tsd = torch.arange(S, dtype=torch.int64, device="cuda") * 50 + 1
    step = torch.tensor([start], dtype=torch.int32, device="cuda")
    tsbuf = torch.full((n_ts + 4,), -5, dtype=torch.int64, device="cuda")
    L.call("ldmk_advance_timestep", step.data_ptr(), tsd.data_ptr(), tsbuf.data_ptr(), n_ts, advance, S, ops.stream())
    assert step.item() == expect
    assert tsbuf.tolist() == [expect * 50 + 1] * n_ts + [-5] * 4


# ------------------------------------------------------------------------------------------ layout helpers
@pytest.mark.parametrize("perm", list(itertools.permutations(range(3))))
def test_permute3_all_permutations(ops, perm):
    """ldmk_permute3: every permutation of a (3, 5, 7) tensor, exact."""
    x = rnd(500, 3, 5, 7)
    assert torch.equal(ops.permute3(x.cuda(), perm).cpu(), x.permute(*perm).contiguous())


def test_permute3_grid_stride(ops):
    """(130, 90, 95) = 1 111 500 elements > 1 048 576, permutation (2, 0, 1), exact."""
    x = rnd(501, 130, 90, 95)
    assert x.numel() > GRID_PASS
    assert torch.equal(ops.permute3(x.cuda(), (2, 0, 1)).cpu(), x.permute(2, 0, 1).contiguous())


def test_pack_conv3x3_grid_stride(ops):
    """ldmk_pack_conv3x3 at 352 x 352 x 9 = 1 115 136 elements: OIHW -> [I/32][9][32][O], exact."""
    w = rnd(502, 352, 352, 3, 3)
    assert w.numel() > GRID_PASS
    ref = w.view(352, 11, 32, 9).permute(1, 3, 2, 0).reshape(9 * 352, 352)
    assert torch.equal(ops.pack_conv3x3(w.cuda()).cpu(), ref)


def _mask_rows_case(ops, L, n, c, h, w, y0, value):
    img = rnd(510 + h, n, c, h, w)
    ref = img.clone()
    for i in range(n):
        ref[i, :, y0[i]:, :] = value
    d, y0d = img.cuda(), torch.tensor(y0, dtype=torch.int32, device="cuda")
    L.call("ldmk_mask_rows", d.data_ptr(), y0d.data_ptr(), n, c, h, w, value, ops.stream())
    assert torch.equal(d.cpu(), ref)


def test_mask_rows(ops, L):
    """ldmk_mask_rows: img[i, :, y0[i]:, :] = value, exact; y0 = 0 (all rows), inside, = h (none)."""
    _mask_rows_case(ops, L, 3, 3, 20, 12, [0, 7, 20], 0.5)


def test_mask_rows_grid_stride(ops, L):
    """2 x 3 x 420 x 420 = 1 058 400 elements > 1 048 576, exact."""
    assert 2 * 3 * 420 * 420 > GRID_PASS
    _mask_rows_case(ops, L, 2, 3, 420, 420, [5, 419], -1.0)


def _add_rowvec_case(ops, rows, c, rps, pad):
    ns = (rows + rps - 1) // rps
    x, vw = rnd(520 + c, rows, c), rnd(521 + c, ns, c + pad)
    ref = (x.double() + vw[:, :c].double().repeat_interleave(rps, 0)[:rows]).float()      # one rounding: exact in fp32
    xd = x.cuda()
    ops.add_rowvec_(xd, vw.cuda()[:, :c], rps)
    assert torch.equal(xd.cpu(), ref)


def test_add_rowvec(ops):
    """ldmk_add_rowvec: x[row] += vec[row / rows_per_sample], vec_ld > c, a rows_per_sample (37) that does not divide the
    256-thread workgroup, a ragged last sample; one fp32 add per element, so exact against the rounded float64 sum."""
    _add_rowvec_case(ops, 3 * 37 - 5, 64, 37, 8)
    _add_rowvec_case(ops, 5, 4, 1, 4)


def test_add_rowvec_grid_stride(ops):
    """The kernel strides over float4s: 16 200 x 260 floats = 1 053 000 float4s > 1 048 576 (16 MB, the smallest size at
    which its loop takes a second pass), exact."""
    assert 16200 * 260 // 4 > GRID_PASS
    _add_rowvec_case(ops, 16200, 260, 4111, 4)


def _postprocess_ref(x):
    return ((x.double() + 1.0) / 2.0).clamp(0.0, 1.0).permute(0, 2, 3, 1).contiguous().float()


def test_postprocess_frames(ops):
    """ldmk_postprocess_frames: NCHW -> NHWC of clamp((x + 1) / 2, 0, 1); inputs below -1, above 1 and exactly +-1; one
    fp32 add and an exact halving per element, so exact against the rounded float64 value."""
    x = rnd(530, 2, 3, 9, 11)
    x[0, 0, 0, :4] = torch.tensor([-1.0, 1.0, -3.5, 2.25])
    assert (x < -1).any() and (x > 1).any()
    got = ops.postprocess_frames(x.cuda()).cpu()
    assert torch.equal(got, _postprocess_ref(x))
    assert got[0, 0, :4, 0].tolist() == [0.0, 1.0, 0.0, 1.0]


def test_postprocess_frames_grid_stride(ops):
    """2 x 3 x 420 x 420 = 1 058 400 elements > 1 048 576, exact."""
    x = rnd(531, 2, 3, 420, 420)
    assert x.numel() > GRID_PASS
    assert torch.equal(ops.postprocess_frames(x.cuda()).cpu(), _postprocess_ref(x))


# ------------------------------------------------------------------------------------------ heads gather / scatter
def _heads_case(ops, n, tokens, heads, d, dp, col0, ld):
    C_ = heads * d
    src = rnd(540 + d + col0, n * tokens, ld)
    ref = torch.zeros(n, heads, tokens, dp)
    ref[..., :d] = src[:, col0:col0 + C_].reshape(n, tokens, heads, d).permute(0, 2, 1, 3)
    g = ops.heads_gather(src.cuda(), col0, n, tokens, heads, d, dp,
                         out=torch.full((n * heads, tokens, dp), SENTINEL, device="cuda"))
    assert torch.equal(g.cpu().view(n, heads, tokens, dp), ref), "gather"
    wide, dst = _padded(n * tokens, C_, 8)
    ops.heads_scatter_(g, dst, n, tokens, heads, d, dp)
    assert torch.equal(dst.cpu(), src[:, col0:col0 + C_]), "scatter of the gather"
    assert torch.all(wide[:, C_:] == SENTINEL), "scatter wrote beyond heads * d columns"


@pytest.mark.parametrize("tokens", [32, 96])
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("d,dp", [(40, 64), (64, 64), (80, 96)])
def test_heads_gather_scatter(ops, d, dp, which, tokens):
    """ldmk_heads_gather from column col0 in {0, C, 2C} of a [q | k | v] tensor: equal to the torch indexing with the d
    columns of a head zero-padded to dp, exactly; ldmk_heads_scatter of that result restores the source columns exactly
    and leaves the other columns of a wider destination untouched."""
    heads = 3
    _heads_case(ops, 2, tokens, heads, d, dp, which * heads * d, 3 * heads * d)


def test_heads_gather_scatter_grid_stride(ops):
    """2 x 2300 tokens x 3 heads: 1 324 800 gathered and 1 104 000 scattered elements, both > 1 048 576, exact."""
    assert 2 * 2300 * 3 * 80 > GRID_PASS
    _heads_case(ops, 2, 2300, 3, 80, 96, 0, 240)


# ------------------------------------------------------------------------------------------ audio attention forward
def _audio_module(T_win):
    from dsml_thesis_amd.encoders import Conv1DTemporalAttention
    from dsml_thesis_amd.synth import load_recipe
    mod = Conv1DTemporalAttention(seq_len=T_win, subspace_dim=768)
    load_recipe(mod)
    return mod


def audio_ref(mod, x, dtype=torch.float64):
    from dsml_thesis_amd.encoders import Conv1DTemporalAttention
    n, T_win, dim = x.shape
    ref = Conv1DTemporalAttention(seq_len=T_win, subspace_dim=dim).to(dtype)
    ref.load_state_dict({k: v.to(dtype) for k, v in mod.state_dict().items()})
    with torch.no_grad():
        xt = x.to(dtype).transpose(1, 2)
        attn = ref.attentionNet(ref.attentionConvNet(xt).view(n, T_win)).view(n, T_win, 1)
        return torch.bmm(xt, attn).view(n, dim).unsqueeze(1)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("T_win", [1, 9, 17, 32])
def test_audio_attention_forward(T_win, n):
    """ldmk_audio_attention at both ends of its window range (T = 1, T = AA_TMAX = 32) and the shipped 9 / 17 frames,
    against the float64 Conv1DTemporalAttention modules with the recipe weights of test_audio_attention_backward;
    bound 2e-5 * max|ref| as there."""
    mod = _audio_module(T_win)
    x = rnd(70 + T_win, n, T_win, 768)
    ref = audio_ref(mod, x)
    _close(mod.cuda()(x.cuda()), ref, 2e-5, f"audio attention forward T={T_win} n={n}")


@pytest.mark.parametrize("T_bad", [0, 33])
def test_audio_attention_rejects_window(ops, L, T_bad):
    """T outside [1, 32] is refused before any launch (every buffer is sized for T = 33)."""
    mod = _audio_module(33).cuda()
    mod._pack()
    x = torch.zeros(1, 33, 768, device="cuda")
    out = torch.zeros(1, 768, device="cuda")
    with pytest.raises(L.LdmkError, match="window T="):
        L.call("ldmk_audio_attention", x.data_ptr(), 1, T_bad, 768, mod._wp.data_ptr(), mod._bp.data_ptr(), mod._lw.data_ptr(),
               mod._lb.data_ptr(), out.data_ptr(), ops.stream())
