"""GPU: the two kernels under `DPMSolverSampler` through the C ABI -- `ldmk_timestep_embedding_f32` and `ldmk_dpm_step` -- against
float64 restatements built from the same fp32 inputs, the same fp32 ring and the same fp32 table.

# Bound of ldmk_dpm_step: derived, per element R * 2^-24 * A.
#   A = the update evaluated in float64 with every term replaced by its absolute value, the inside of m0 included:
#       m0 -> (|x| + sigma_s (|e_u| + |scale| (|e_c| + |e_u|))) / alpha_s, differences -> sums of absolute values.
#   R = 14 = the number of fp32 roundings on the longest chain of the kernel (order 3 under guidance):
#       e = e_u + scale (e_c - e_u)            3   (sub, mul, add)
#       m0 = (x - sigma_s e) / alpha_s         3   (mul, sub, div)
#       D1_0 = (1/r0) (m0 - m1)                2   (sub, mul)
#       D1_0 - D1_1                            1
#       D1 = D1_0 + q (D1_0 - D1_1)            2   (mul, add)
#       c_1 D1                                 1
#       (c_x x - c_0 m0) + c_1 D1              1
#       ... - c_2 D2                           1
#     Every other chain (through c_x x, c_0 m0, D1_1, D2, and all of orders 1 and 2) is shorter.  Each rounding perturbs a partial
#     result by at most 2^-24 relative, and every partial result is bounded by its part of A.  The same R holds every case.
#   The ring slot and pred_x0 (m0 itself: 6 roundings) are held to 6 * 2^-24 * A_m0.
# alpha_s, sigma_s are those of the real schedule's FIRST step (t = 1: alpha = 0.0098 on this schedule, the smallest there is) in every
# row: m0 is largest there, ~100 |x|, and the past predictions in the ring are drawn at that magnitude.
# Worst measured ratio to the bound is printed per test (DESIGN section 19 records it)."""
import numpy as np
import pytest
import torch

from conftest import rnd
from oracle import ldm_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GRID_PASS = 256 * 4096
R, R_M0 = 14, 6
U = 2.0 ** -24
S = 7
ROW = 12


@pytest.fixture(scope="module")
def L():
    from dsml_thesis_amd import lib
    lib.load()
    return lib


@pytest.fixture(scope="module")
def tab():
    """The real S = 7, order-3 table (orders 1, 2, 3, 3, 3, 3, 3: rows 2.. carry every coefficient) with the first step's alpha_s and
    sigma_s in every row."""
    from dsml_thesis_amd.dpm_solver import step_table
    t = step_table(O.register_schedule(**W.SCHEDULE)["alphas_cumprod"], S, order=3, lower_order_final=False)
    assert t.orders == [1, 2, 3, 3, 3, 3, 3]
    table = t.table.clone()
    assert 0 < table[0, 0] == table[:, 0].min() < 0.02, table[:, 0]
    table[:, 0], table[:, 1] = table[0, 0], table[0, 1]
    return table


# ------------------------------------------------------------------------------------------ float64 restatement
def step64(x, eps, ring, row, k, cfg, scale):
    """x [total], eps [total or 2 total], ring [3][total] fp32 -> (x', m0, A, A_m0) in float64 (dpm_solver.py:340-344, 386-399,
    526-533, 783-790, 835-849 from one fp32 table row)."""
    total = x.shape[0]
    x, eps, ring, r = x.astype(np.float64), eps.astype(np.float64), ring.astype(np.float64), row.astype(np.float64)
    ax = np.abs(x)
    if cfg:
        eu, ec, s = eps[:total], eps[total:], np.float64(np.float32(scale))
        e, ae = eu + s * (ec - eu), np.abs(eu) + abs(s) * (np.abs(ec) + np.abs(eu))
    else:
        e, ae = eps[:total], np.abs(eps[:total])
    al, sg, o, cx, c0, ir0, ir1, q, irs, c1, c2 = r[:11]
    m0, am0 = (x - sg * e) / al, (ax + sg * ae) / al
    m1, m2 = ring[(k + 2) % 3], ring[(k + 1) % 3]
    xt, A = cx * x - c0 * m0, cx * ax + abs(c0) * am0
    if o == 2:
        xt = xt - (0.5 * c0) * (ir0 * (m0 - m1))
        A = A + abs(0.5 * c0) * (abs(ir0) * (am0 + np.abs(m1)))
    elif o == 3:
        d10, d11 = ir0 * (m0 - m1), ir1 * (m1 - m2)
        a10, a11 = abs(ir0) * (am0 + np.abs(m1)), abs(ir1) * (np.abs(m1) + np.abs(m2))
        d1, d2 = d10 + q * (d10 - d11), irs * (d10 - d11)
        a1, a2 = a10 + abs(q) * (a10 + a11), abs(irs) * (a10 + a11)
        xt = xt + c1 * d1 - c2 * d2
        A = A + abs(c1) * a1 + abs(c2) * a2
    return xt, m0, A, am0


def within(got, ref, A, rounds, what):
    got = got.detach().cpu().double().numpy().reshape(-1)
    err, bound = np.abs(got - ref), rounds * U * A
    ratio = float((err / bound).max())
    print(f"  {what}: max |err| {err.max():.3e}, worst ratio to {rounds} * 2^-24 * A: {ratio:.3f} (|ref| up to {np.abs(ref).max():.3g})")
    assert np.all(err <= bound), (what, ratio)
    return ratio


# ------------------------------------------------------------------------------------------ device side
class Dev:
    """The device buffers of one case, each followed by sentinel words that no launch may touch."""

    def __init__(self, total, n_ts=5):
        self.total, self.n_ts = total, n_ts
        self.ring, self.xp, self.p0 = self.buf(3 * total), self.buf(total), self.buf(total)
        self.ts = self.buf(n_ts)
        self.step = torch.zeros(1, dtype=torch.int32, device="cuda")

    @staticmethod
    def buf(n):
        return torch.full((n + 8,), SENTINEL, device="cuda")

    def guards_intact(self):
        t = self.total
        return all(bool(torch.all(b[n:] == SENTINEL)) for b, n in ((self.ring, 3 * t), (self.xp, t), (self.p0, t), (self.ts, self.n_ts)))


def launch(L, table, d, x, eps, n, cfg=0, scale=1.0, x_prev=None, pred_x0=True, advance=0, max_order=3):
    x_prev = d.xp if x_prev is None else x_prev
    L.call("ldmk_dpm_step", x.data_ptr(), eps.data_ptr(), table.data_ptr(), d.step.data_ptr(), float(scale), int(cfg), d.ring.data_ptr(),
           x_prev.data_ptr(), d.p0.data_ptr() if pred_x0 else 0, d.total // n, n, d.ts.data_ptr() if advance else 0,
           d.n_ts if advance else 0, advance, table.shape[0], max_order, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def one_launch_case(L, tab, order, cfg, n, per, k=3, seed=300):
    """Row k with its order set to `order`; a full ring of past predictions at the magnitude m0 has at the first step's alpha."""
    total, scale = n * per, 3.0
    table = tab.clone()
    table[k, 2] = float(order)
    row = table[k].numpy()
    table = table.cuda()
    x, eps = rnd(seed, total), rnd(seed + 1, (2 if cfg else 1) * total)
    ring = rnd(seed + 2, 3, total) / tab[0, 0]
    d = Dev(total)
    d.step.fill_(k)
    d.ring[:3 * total] = ring.reshape(-1).cuda()
    xd, ed = x.cuda(), eps.cuda()
    launch(L, table, d, xd, ed, n, cfg, scale)
    xt, m0, A, am0 = step64(x.numpy(), eps.numpy(), ring.numpy(), row, k, cfg, scale)
    tag = f"order {order} cfg {cfg} n {n} per {per}"
    ratio = within(d.xp[:total], xt, A, R, tag + " x'")
    within(d.p0[:total], m0, am0, R_M0, tag + " pred_x0")
    got_ring = d.ring[:3 * total].view(3, total).cpu()
    assert torch.equal(got_ring[k % 3], d.p0[:total].cpu()), "m0 goes to slot k % 3"
    for s_ in ((k + 1) % 3, (k + 2) % 3):
        assert torch.equal(got_ring[s_], ring[s_]), "the two other slots stay"
    assert int(d.step.item()) == k and bool(torch.all(d.ts == SENTINEL)), "advance = 0 moves nothing"
    assert d.guards_intact()
    first = d.xp[:total].clone()
    # the same launch again, x' aliasing x, no pred_x0: the same bits
    d.ring[:3 * total] = ring.reshape(-1).cuda()
    d.p0.fill_(SENTINEL)
    xa = torch.cat([xd, torch.full((8,), SENTINEL, device="cuda")])
    launch(L, table, d, xa, ed, n, cfg, scale, x_prev=xa, pred_x0=False)
    assert torch.equal(xa[:total], first), "x' aliasing x, pred_x0 absent: bit for bit the first launch"
    assert bool(torch.all(xa[total:] == SENTINEL)) and bool(torch.all(d.p0 == SENTINEL)) and d.guards_intact()
    return ratio


@pytest.mark.parametrize("per", [1, 63, 256])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("cfg", [0, 1], ids=["plain", "cfg3"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_one_step(L, tab, order, cfg, n, per):
    one_launch_case(L, tab, order, cfg, n, per)


def test_one_step_longer_than_a_full_grid(L, tab):
    """4096 blocks x 256 threads + 77 elements: the grid-stride loop iterates (order 3 under guidance, the longest chain)."""
    one_launch_case(L, tab, 3, 1, 1, GRID_PASS + 77, seed=320)


def test_an_order_1_row_never_reads_the_ring(L, tab):
    total, n = 3 * 63, 3
    d = Dev(total)
    d.ring[:3 * total] = float("nan")
    x, eps = rnd(330, total), rnd(331, total)
    launch(L, tab.cuda(), d, x.cuda(), eps.cuda(), n)                 # step_idx = 0: row 0, order 1
    assert bool(torch.isfinite(d.xp[:total]).all())
    xt, _, A, _ = step64(x.numpy(), eps.numpy(), np.zeros((3, total), np.float32), tab[0].numpy(), 0, 0, 1.0)
    within(d.xp[:total], xt, A, R, "row 0 over a ring of NaN")


def test_seven_chained_steps_at_order_3(L, tab):
    """Orders 1, 2, 3, 3, 3, 3, 3 from step_idx = 0 with the advance, n_ts = 5 != n = 3: the ring wraps twice.  Every step is compared
    from the kernel's own state before it (latent, ring), so the bound is the one-step bound; the model time written to all n_ts
    entries is row k's, step_idx goes up by one, and a launch past the end stays on the last row."""
    n, per, scale = 3, 63, 3.0
    total = n * per
    table = tab.cuda()
    d = Dev(total, n_ts=5)
    d.ring[:3 * total] = float("nan")                      # dead contents: the orders 1, 2 of rows 0, 1 never read them
    x = torch.cat([rnd(340, total).cuda(), torch.full((8,), SENTINEL, device="cuda")])
    worst = 0.0
    for k in range(S):
        eps = rnd(341 + k, 2 * total)
        x_before, ring_before = x[:total].cpu().numpy(), np.nan_to_num(d.ring[:3 * total].view(3, total).cpu().numpy())
        launch(L, table, d, x, eps.cuda(), n, 1, scale, x_prev=x, advance=1)
        xt, m0, A, am0 = step64(x_before, eps.numpy(), ring_before, tab[k].numpy(), k, 1, scale)
        worst = max(worst, within(x[:total], xt, A, R, f"step {k} x'"))
        within(d.ring[:3 * total].view(3, total)[k % 3], m0, am0, R_M0, f"step {k} ring slot {k % 3}")
        assert int(d.step.item()) == k + 1
        assert d.ts[:5].cpu().tolist() == [tab[k, 11].item()] * 5, "all n_ts entries = the model time of t_{k+1}"
        assert d.guards_intact() and bool(torch.all(x[total:] == SENTINEL))
    print(f"  worst ratio over the chain: {worst:.3f}")
    assert bool(torch.isfinite(d.ring[:3 * total]).all())
    before = x[:total].clone()
    launch(L, table, d, x, rnd(360, 2 * total).cuda(), n, 1, scale, x_prev=x, advance=1)
    assert int(d.step.item()) == S and d.guards_intact(), "past the end: the last row again, no index beyond the table"
    assert not torch.equal(before, x[:total])


# ------------------------------------------------------------------------------------------ the real-valued timestep embedding
def freqs_for(dim):
    half = dim // 2
    return torch.exp(-np.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)


def embed(L, name, t, dim):
    f = freqs_for(dim).cuda()
    n = t.shape[0]
    out = torch.full((n * dim + 8,), SENTINEL, device="cuda")
    L.call(name, t.data_ptr(), f.data_ptr(), out.data_ptr(), n, dim, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool(torch.all(out[n * dim:] == SENTINEL))
    return out[:n * dim].view(n, dim).cpu()


@pytest.mark.parametrize("dim", [32, 33])
@pytest.mark.parametrize("reps", [1, 10], ids=["one-block", "three-blocks"])
def test_timestep_embedding_f32_against_float64(L, dim, reps):
    """arg = t * f in fp32 (as the reference, util.py:161-165), cos and sin of it in float64, rounded once.  The restatement does the
    same; two correctly-rounded results of |.| <= 1 differ by at most one fp32 ulp below 1, 2^-24 -- held to 2^-23."""
    t = torch.tensor([0.0, 0.5, 799.2, 999.0] * reps, dtype=torch.float32)
    got = embed(L, "ldmk_timestep_embedding_f32", t.cuda(), dim)
    half = dim // 2
    arg = (t.numpy()[:, None] * freqs_for(dim).numpy()[None]).astype(np.float32).astype(np.float64)
    ref = np.concatenate([np.cos(arg), np.sin(arg)] + ([np.zeros((t.shape[0], 1))] if dim % 2 else []), axis=1)
    assert got.shape == ref.shape == (4 * reps, dim) and 2 * half + dim % 2 == dim
    err = np.abs(got.double().numpy() - ref).max()
    print(f"  dim {dim}: max |err| {err:.3e}")
    assert err <= 2.0 ** -23
    if dim % 2:
        assert bool(torch.all(got[:, -1] == 0))


@pytest.mark.parametrize("dim", [32, 33])
def test_timestep_embedding_f32_is_bitwise_the_int64_kernel_at_integer_times(L, dim):
    ti = torch.tensor([0, 1, 2, 250, 499, 799, 998, 999] * 5, dtype=torch.int64)
    a = embed(L, "ldmk_timestep_embedding", ti.cuda(), dim)
    b = embed(L, "ldmk_timestep_embedding_f32", ti.to(torch.float32).cuda(), dim)
    assert torch.equal(a, b)
