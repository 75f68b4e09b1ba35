"""GPU: `ldmk_plms_step` through the C ABI against a float64 numpy restatement of plms.py:199-236 built from the same fp32 inputs
and the same fp32 table row.

Bound: rtol = atol = 2e-5 against float64, the bound `test_use_original_steps_walks_the_models_own_schedule` holds the DDIM update
to.  The update here adds the Adams-Bashforth combination in front of it: at most four products of |e| <= 5 by 55, 59, 37, 9 and
three sums, each rounded at a magnitude below 512 (half an ulp: 1.5e-5), then divided by 24 -- under 3e-6 in e', which the update
multiplies by |sqrt(1 - a_prev) - sqrt(a_prev) sqrt(1 - a_t) / sqrt(a_t)| < 1 and, for pred_x0, by sqrt(1 - a_t) / sqrt(a_t) < 6.4 at
the schedule indices used (S = 20, indices 0-13), where |pred_x0| grows by the same factor.  A plain fp32 numpy evaluation of the
same formula uses at most 0.22 of the bound on the single launches and 0.66 at the end of the seven chained steps (whose
float64 recursion runs on its own, so the differences add up).

Shapes: per_sample = 105, n = 3 (315 elements: one full block and a partial one, odd for any vector width) and one total just
above one pass of a `grid_for()` launch (4096 blocks x 256 threads + 77), where the grid-stride loop iterates."""
import numpy as np
import pytest
import torch

from conftest import rnd
from oracle import ldm_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GRID_PASS = 256 * 4096
S = 20
N, PER = 3, 105
MULTISTEP, PREDICTOR, CORRECTOR = 0, 1, 2
TOL = 2e-5


@pytest.fixture(scope="module")
def L():
    from dsml_thesis_amd import lib
    lib.load()
    return lib


@pytest.fixture(scope="module")
def sched():
    from dsml_thesis_amd import schedule as S_
    ac = torch.as_tensor(O.register_schedule(**W.SCHEDULE)["alphas_cumprod"]).cpu()
    ts = O.make_ddim_timesteps(S)
    tab = S_.ddim_step_table(ac, ts, 0.0)                     # [S][4] float32: a_t, a_prev, sigma (0), sqrt(1 - a_t)
    return dict(tab=np.asarray(tab), ts=ts.astype(np.int64), table=torch.from_numpy(np.asarray(tab)).cuda(),
                tsd=torch.from_numpy(ts.astype(np.int64)).cuda())


# ------------------------------------------------------------------------------------------ float64 restatement
def combine64(e, olds, count):
    """plms.py:224-232; `olds` newest first"""
    if count == 0:
        return e
    if count == 1:
        return (3 * e - olds[0]) / 2
    if count == 2:
        return (23 * e - 16 * olds[0] + 5 * olds[1]) / 12
    return (55 * e - 59 * olds[0] + 37 * olds[1] - 9 * olds[2]) / 24


def update64(x, ep, row):
    """get_x_prev_and_pred_x0, plms.py:199-216 with sigma = 0, from one fp32 table row"""
    a_t, a_prev, s1m = np.float64(row[0]), np.float64(row[1]), np.float64(row[3])
    p0 = (x - s1m * ep) / np.sqrt(a_t)
    return np.sqrt(a_prev) * p0 + np.sqrt(1.0 - a_prev) * ep, p0


def guided64(eps, cfg, scale, total):
    eps = eps.reshape(-1).astype(np.float64)
    return eps[:total] + np.float64(np.float32(scale)) * (eps[total:] - eps[:total]) if cfg else eps[:total]


def close(got, ref, what=""):
    got = got.detach().cpu().double().reshape(-1)
    ref = torch.from_numpy(np.asarray(ref, dtype=np.float64)).reshape(-1)
    err = (got - ref).abs().max().item()
    print(f"  {what}: max |err| {err:.3e} (|ref| up to {ref.abs().max().item():.3g})")
    torch.testing.assert_close(got, ref, rtol=TOL, atol=TOL)


# ------------------------------------------------------------------------------------------ device side
class Dev:
    """The device buffers of one case, each followed by sentinel words that no launch may touch."""

    def __init__(self, total, n_ts=5):
        self.total, self.n_ts = total, n_ts
        self.ring = self.buf(3 * total)
        self.keep, self.xp, self.p0 = self.buf(total), self.buf(total), self.buf(total)
        self.ts = torch.full((n_ts + 4,), -5, dtype=torch.int64, device="cuda")
        self.step = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.count = torch.zeros(1, dtype=torch.int32, device="cuda")
        self._guarded = []

    @staticmethod
    def buf(n):
        return torch.full((n + 8,), SENTINEL, device="cuda")

    def slot(self, k):
        return self.ring[k * self.total:(k + 1) * self.total]

    def load(self, index, olds, count):
        """The `count` newest of `olds` (newest first) where the kernel expects them: the output of index + j in slot (index + j) % 3."""
        self.step.fill_(index)
        self.count.fill_(count)
        self.ring[:3 * self.total] = SENTINEL              # a slot the order does not cover must not reach the result
        for j in range(1, count + 1):
            self.slot((index + j) % 3).copy_(olds[j - 1].reshape(-1))

    def guards_intact(self):
        t = self.total
        return all(bool(torch.all(b[n:] == SENTINEL)) for b, n in ((self.ring, 3 * t), (self.keep, t), (self.xp, t), (self.p0, t))) \
            and self.ts[self.n_ts:].tolist() == [-5] * 4


def launch(L, sched, d, x, eps, mode, cfg=0, scale=1.0, x_prev=None, pred_x0="own", keep="own", advance=0, n=N):
    x_prev = d.xp if x_prev is None else x_prev
    p0 = d.p0.data_ptr() if isinstance(pred_x0, str) else 0
    kp = d.keep.data_ptr() if isinstance(keep, str) else 0
    L.call("ldmk_plms_step", x.data_ptr(), eps.data_ptr(), sched["table"].data_ptr(), d.step.data_ptr(), d.count.data_ptr(),
           float(scale), int(cfg), mode, d.ring.data_ptr(), kp, x_prev.data_ptr(), p0, d.total // n, n,
           sched["tsd"].data_ptr() if advance else 0, d.ts.data_ptr() if advance else 0, d.n_ts if advance else 0, advance,
           S if advance else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def inputs(seed, total, cfg):
    x = rnd(seed, total)
    eps = rnd(seed + 1, (2 if cfg else 1) * total)
    olds = [0.9 * rnd(seed + 2 + j, total) for j in range(3)]
    return x, eps, olds


# ------------------------------------------------------------------------------------------ multistep, counts 0-3
@pytest.mark.parametrize("cfg", [0, 1], ids=["plain", "cfg"])
@pytest.mark.parametrize("count", [0, 1, 2, 3])
def test_multistep_orders(L, sched, count, cfg):
    """One launch per order, no advance: x_prev, pred_x0 and the stored e_t against float64; the two other ring slots, the count
    and the counter stay as they were; then pred_x0 = NULL with x_prev aliasing x gives the same x_prev bit for bit."""
    total, index, scale = N * PER, 7, 3.0
    x, eps, olds = inputs(100 + 10 * count, total, cfg)
    d = Dev(total)
    d.load(index, [o.cuda() for o in olds], count)
    before = d.ring.clone()
    xd, ed = x.cuda(), eps.cuda()
    launch(L, sched, d, xd, ed, MULTISTEP, cfg, scale)
    e64 = guided64(eps.numpy(), cfg, scale, total)
    ep = combine64(e64, [o.numpy().astype(np.float64) for o in olds], count)
    rx, rp = update64(x.numpy().astype(np.float64), ep, sched["tab"][index])
    close(d.xp[:total], rx, f"order {count + 1} x_prev")
    close(d.p0[:total], rp, f"order {count + 1} pred_x0")
    close(d.slot(index % 3), e64, "stored e_t")
    for k in ((index + 1) % 3, (index + 2) % 3):
        assert torch.equal(d.slot(k), before[k * total:(k + 1) * total]), "only e_t's slot is written"
    assert d.step.item() == index and d.count.item() == count and d.guards_intact()
    assert d.ts[:d.n_ts].tolist() == [-5] * d.n_ts, "advance = 0 leaves the timestep vector alone"
    # again from the same state: in place, without pred_x0
    first = d.xp[:total].clone()
    d.load(index, [o.cuda() for o in olds], count)
    d.p0.fill_(SENTINEL)
    xa = torch.cat([xd, torch.full((8,), SENTINEL, device="cuda")])
    launch(L, sched, d, xa, ed, MULTISTEP, cfg, scale, x_prev=xa, pred_x0=None)
    assert torch.equal(xa[:total], first) and torch.all(xa[total:] == SENTINEL) and torch.all(d.p0 == SENTINEL)


def test_seven_chained_steps_wrap_the_ring_twice(L, sched):
    """Seven multistep launches with the advance, guidance on, from an empty ring: orders 1, 2, 3, 4, 4, 4, 4, seven stores into three
    slots.  Every step against the float64 recursion (which runs on its own from the start values), and after each step the
    counter, the timestep vector and the count."""
    total, scale, index = N * PER, 3.0, 13
    x = rnd(200, total)
    d = Dev(total)
    d.load(index, [], 0)
    xd = x.cuda()
    x64, olds64 = x.numpy().astype(np.float64), []
    for k in range(7):
        eps = rnd(210 + k, 2 * total)
        launch(L, sched, d, xd, eps.cuda(), MULTISTEP, 1, scale, x_prev=xd, advance=1)
        e64 = guided64(eps.numpy(), 1, scale, total)
        x64, p64 = update64(x64, combine64(e64, olds64, min(len(olds64), 3)), sched["tab"][index])
        olds64 = [e64] + olds64[:2]
        close(xd, x64, f"step {k} x_prev")
        close(d.p0[:total], p64, f"step {k} pred_x0")
        index -= 1
        assert d.step.item() == index and d.count.item() == min(k + 1, 3)
        assert d.ts[:d.n_ts].tolist() == [int(sched["ts"][index])] * d.n_ts and d.guards_intact()
    for j, e64 in enumerate(olds64, start=1):                 # the ring holds the last three outputs, newest at (index + 1) % 3
        close(d.slot((index + j) % 3), e64, f"ring entry -{j}")


# ------------------------------------------------------------------------------------------ the Euler step
@pytest.mark.parametrize("cfg", [0, 1], ids=["plain", "cfg"])
@pytest.mark.parametrize("index", [0, 6])
def test_predictor(L, sched, index, cfg):
    """x_prev = the DDIM update with e_t, in place in x's buffer; x itself goes to the keep buffer bit for bit; e_t goes to the ring;
    neither the counter nor the count moves; ts = the timestep of max(index - 1, 0) -- at index 0 the same timestep."""
    total, scale = N * PER, 3.0
    x, eps, _ = inputs(300 + index, total, cfg)
    d = Dev(total)
    d.load(index, [], 0)
    d.count.fill_(2)                                          # (whatever it holds, the predictor ignores and keeps it)
    xd = x.cuda()
    launch(L, sched, d, xd, eps.cuda(), PREDICTOR, cfg, scale, x_prev=xd, advance=1)
    e64 = guided64(eps.numpy(), cfg, scale, total)
    rx, rp = update64(x.numpy().astype(np.float64), e64, sched["tab"][index])
    close(xd, rx, "predicted x")
    close(d.p0[:total], rp, "predictor pred_x0")
    close(d.slot(index % 3), e64, "stored e_t")
    assert torch.equal(d.keep[:total].cpu(), x), "the original latent is kept"
    assert d.step.item() == index and d.count.item() == 2
    assert d.ts[:d.n_ts].tolist() == [int(sched["ts"][max(index - 1, 0)])] * d.n_ts and d.guards_intact()
    assert torch.all(d.slot((index + 1) % 3) == SENTINEL) and torch.all(d.slot((index + 2) % 3) == SENTINEL)


@pytest.mark.parametrize("cfg", [0, 1], ids=["plain", "cfg"])
def test_corrector(L, sched, cfg):
    """e' = (e_t from the ring + e_next) / 2 applied to the KEPT latent; the ring keeps e_t; the advance sets the count to 1."""
    total, scale, index = N * PER, 3.0, 6
    x, eps, olds = inputs(320, total, cfg)
    d = Dev(total)
    d.load(index, [], 0)
    d.slot(index % 3).copy_(olds[0].cuda())                   # e_t, as the predictor left it
    before = d.ring.clone()
    launch(L, sched, d, x.cuda(), eps.cuda(), CORRECTOR, cfg, scale, keep=None, advance=1)
    e_next = guided64(eps.numpy(), cfg, scale, total)
    rx, rp = update64(x.numpy().astype(np.float64), (olds[0].numpy().astype(np.float64) + e_next) / 2, sched["tab"][index])
    close(d.xp[:total], rx, "corrected x_prev")
    close(d.p0[:total], rp, "corrected pred_x0")
    assert torch.equal(d.ring, before), "the ring keeps e_t, not e_next"
    assert d.step.item() == index - 1 and d.count.item() == 1
    assert d.ts[:d.n_ts].tolist() == [int(sched["ts"][index - 1])] * d.n_ts and d.guards_intact()
    assert torch.all(d.keep == SENTINEL)


def test_euler_then_multistep_is_the_loop(L, sched):
    """Predictor, corrector and two multistep launches chained on device state alone -- the sampler's first three steps."""
    total, index = N * PER, 9
    x = rnd(400, total)
    es = [rnd(401 + k, total) for k in range(4)]
    d = Dev(total)
    d.load(index, [], 0)
    xd = x.cuda()
    launch(L, sched, d, xd, es[0].cuda(), PREDICTOR, x_prev=xd, advance=1)
    launch(L, sched, d, d.keep, es[1].cuda(), CORRECTOR, x_prev=xd, keep=None, advance=1)
    f = lambda a: a.numpy().astype(np.float64)
    x64, _ = update64(f(x), (f(es[0]) + f(es[1])) / 2, sched["tab"][index])
    close(xd, x64, "after the Euler step")
    olds = [f(es[0])]
    for k in (2, 3):
        index -= 1
        assert d.step.item() == index and d.count.item() == len(olds)
        launch(L, sched, d, xd, es[k].cuda(), MULTISTEP, x_prev=xd, advance=1)
        x64, _ = update64(x64, combine64(f(es[k]), olds, len(olds)), sched["tab"][index])
        olds = [f(es[k])] + olds
        close(xd, x64, f"after multistep {k - 1}")


# ------------------------------------------------------------------------------------------ past one grid pass
@pytest.mark.parametrize("cfg", [0, 1], ids=["plain", "cfg"])
def test_grid_stride(L, sched, cfg):
    """1 048 576 + 77 elements: the grid-stride loop iterates; every element is written once and nothing behind the buffers."""
    total, index, scale = GRID_PASS + 77, 11, 3.0
    x, eps, olds = inputs(500, total, cfg)
    d = Dev(total, n_ts=300)
    d.load(index, [o.cuda() for o in olds], 3)
    launch(L, sched, d, x.cuda(), eps.cuda(), MULTISTEP, cfg, scale, advance=1, n=1)
    e64 = guided64(eps.numpy(), cfg, scale, total)
    rx, rp = update64(x.numpy().astype(np.float64), combine64(e64, [o.numpy().astype(np.float64) for o in olds], 3), sched["tab"][index])
    close(d.xp[:total], rx, "x_prev")
    close(d.p0[:total], rp, "pred_x0")
    close(d.slot(index % 3), e64, "stored e_t")
    assert d.step.item() == index - 1 and d.count.item() == 3
    assert d.ts[:300].tolist() == [int(sched["ts"][index - 1])] * 300 and d.guards_intact()


def test_same_launch_same_bits(L, sched):
    total, index = N * PER, 5
    x, eps, olds = inputs(600, total, 1)
    outs = []
    for _ in range(2):
        d = Dev(total)
        d.load(index, [o.cuda() for o in olds], 3)
        launch(L, sched, d, x.cuda(), eps.cuda(), MULTISTEP, 1, 3.0)
        outs.append((d.xp.clone(), d.p0.clone(), d.ring.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_bad_arguments_are_refused(L, sched):
    d = Dev(N * PER)
    x = torch.zeros(N * PER, device="cuda")
    with pytest.raises(L.LdmkError, match="mode"):
        launch(L, sched, d, x, x, 3)
    with pytest.raises(L.LdmkError, match="advance"):
        launch(L, sched, d, x, x, MULTISTEP, advance=-1)
    with pytest.raises(L.LdmkError, match="bad args"):
        L.call("ldmk_plms_step", x.data_ptr(), x.data_ptr(), sched["table"].data_ptr(), d.step.data_ptr(), 0, 1.0, 0, 0, d.ring.data_ptr(),
               0, d.xp.data_ptr(), 0, PER, N, 0, 0, 0, 0, 0, None)
