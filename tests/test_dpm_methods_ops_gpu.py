"""GPU: the kernels under `DPM_Solver` through the C ABI -- `ldmk_abs_quantile_rows`, `ldmk_dpm_predict_x0`, `ldmk_dpm_stage`.

# ldmk_abs_quantile_rows: bit for bit `abs_quantile_rows_ref` (tests/dpm_methods_cases.py), the fp32 restatement that
#   tests/test_dpm_methods_cpu.py holds to torch.quantile on the CPU bit for bit.
# ldmk_dpm_stage: per element R * 2^-24 * A against a float64 restatement built from the same fp32 inputs, the same fp32 keep / ring
#   buffers and the same fp32 table row.  R is the number of fp32 roundings on the longest chain of the row's kind, counted in the
#   header of `stage64` (tests/dpm_methods_cases.py: kind 0, 4: 8;  kind 1, 2: 9;  kind 3: 14;  kind 5: 10;  kind 6: 14;  kind 7: 6;
#   m itself, which goes to model_out, the ring and the keep slots: 6), A the update with every term replaced by its absolute value.
#   The rows are those of the real tables (both forms, both solver types, singlestep order 3 and multistep order 3).
# Worst measured ratios to the bound are printed per test (DESIGN section 24 records them)."""
import numpy as np
import pytest
import torch

from conftest import rnd
from dpm_methods_cases import ROUNDS, ROUNDS_M, U, abs_quantile_rows_ref, stage64
from oracle import ldm_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GRID_PASS = 256 * 4096


@pytest.fixture(scope="module")
def L():
    from dsml_thesis_amd import lib
    lib.load()
    return lib


def guarded(n, fill=SENTINEL):
    t = torch.full((n + 8,), SENTINEL, device="cuda")
    t[:n] = fill
    return t


def guard_ok(t, n):
    return bool(torch.all(t[n:] == SENTINEL))


# ------------------------------------------------------------------------------------------ the quantile
def quantile(L, v, q, floor_val):
    rows, per = v.shape
    vd = torch.from_numpy(v).cuda().contiguous()
    out = guarded(rows)
    L.call("ldmk_abs_quantile_rows", vd.data_ptr(), rows, per, float(q), float(floor_val), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guard_ok(out, rows), "the guard words after s_out are unchanged"
    return out[:rows].cpu().numpy()


def same_bits(got, ref):
    nan = np.isnan(ref)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32))


PERS = [1, 2, 3, 200, 201, 202, 255, 256, 257, 3072, 3073, 16385]


@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("rows", [1, 3])
def test_abs_quantile_rows_on_normal_data(L, rows, per):
    v = (rnd(1000 + per, rows, per) * 40).numpy()
    for q, floor_val in ((0.995, 1.0), (0.5, 0.0), (0.37, 1e-3), (0.0, 0.0), (1.0, 0.25)):
        got, ref = quantile(L, v, q, floor_val), abs_quantile_rows_ref(v, q, floor_val)
        assert same_bits(got, ref), (rows, per, q, got, ref)


@pytest.mark.parametrize("per", PERS)
def test_abs_quantile_rows_on_special_rows(L, per):
    rs = np.random.RandomState(1100 + per)
    tied = rs.standard_normal(per)
    tied[np.argsort(np.abs(tied))[int(0.9 * per):]] = -3.25                              # heavy ties at the selected rank
    zeros = np.zeros(per)
    zeros[::2] = -0.0
    zeros[1::3] = 1e-41                                                                 # +-0 and denormals
    zeros[2::5] = -3e-45
    nan = rs.standard_normal(per)
    nan[per // 2] = np.nan
    inf = rs.standard_normal(per)
    inf[0] = -np.inf                                                                    # the top rank is inf
    v = np.stack([np.full(per, -2.5), tied, zeros, rs.standard_normal(per) * 1e-3, np.round(rs.standard_normal(per) * 2) / 2, nan,
                  inf]).astype(np.float32)
    for q, floor_val in ((0.995, 1.0), (0.5, 0.0), (1.0, 0.0)):
        got, ref = quantile(L, v, q, floor_val), abs_quantile_rows_ref(v, q, floor_val)
        assert np.isnan(got[5]), "a row holding a NaN gives NaN"
        assert same_bits(got, ref), (per, q, got, ref)
        if q == 0.995:
            assert got[3] == 1.0, "a row entirely below floor_val gives floor_val"
    all_inf = np.full((1, per), -np.inf, np.float32)
    assert np.isnan(quantile(L, all_inf, 0.995 if per > 1 else 1.0, 1.0)[0]) == np.isnan(abs_quantile_rows_ref(all_inf, 0.995 if per > 1 else 1.0, 1.0)[0])


# ------------------------------------------------------------------------------------------ the stage kernel
def tables():
    """(predict_x0, solver_type, method) -> the real table: singlestep order 3 (kinds 0 1 2|3, 0 2, 0) or multistep order 3 with
    lower_order_final off (kinds 4 5 6 6 6 6), plus the denoise_to_zero row (kind 7)."""
    from dsml_thesis_amd.dpm_solver import method_table
    ac = O.register_schedule(**W.SCHEDULE)["alphas_cumprod"]
    out = {}
    for x0 in (True, False):
        for st in ("dpm_solver", "taylor"):
            for method in ("singlestep", "multistep"):
                out[(x0, st, method)] = method_table(ac, steps=6, order=3, method=method, predict_x0=x0, solver_type=st,
                                                     lower_order_final=False, denoise_to_zero=True)
    return out


@pytest.fixture(scope="module")
def tabs():
    return tables()


class Dev:
    """The device buffers of one case, each followed by sentinel words that no launch may touch."""

    def __init__(self, total, n_ts=5):
        self.total, self.n_ts = total, n_ts
        self.keep, self.ring, self.xp, self.out, self.ts = guarded(3 * total), guarded(3 * total), guarded(total), guarded(total), guarded(n_ts)
        self.step = torch.zeros(1, dtype=torch.int32, device="cuda")

    def guards_intact(self):
        t = self.total
        return all(guard_ok(b, n) for b, n in ((self.keep, 3 * t), (self.ring, 3 * t), (self.xp, t), (self.out, t), (self.ts, self.n_ts)))


def launch(L, table, d, x, eps, n, cfg=0, scale=1.0, x_prev=None, out=True, advance=0, uses=3, x0_pre=None, s=None):
    x_prev = d.xp if x_prev is None else x_prev
    L.call("ldmk_dpm_stage", x.data_ptr(), eps.data_ptr(), table.data_ptr(), d.step.data_ptr(), float(scale), int(cfg),
           0 if x0_pre is None else x0_pre.data_ptr(), 0 if s is None else s.data_ptr(), d.keep.data_ptr(), d.ring.data_ptr(),
           x_prev.data_ptr(), d.out.data_ptr() if out else 0, d.total // n, n, d.ts.data_ptr() if advance else 0, d.n_ts if advance else 0,
           advance, table.shape[0], uses, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def within(got, ref, A, rounds, what):
    got = got.detach().cpu().double().numpy().reshape(-1)
    err, bnd = np.abs(got - ref), rounds * U * A
    ratio = float((err / np.maximum(bnd, 1e-300)).max())
    print(f"  {what}: max |err| {err.max():.3e}, worst ratio to {rounds} * 2^-24 * A: {ratio:.3f} (|ref| up to {np.abs(ref).max():.3g})")
    assert np.all(err <= bnd), (what, ratio)
    return ratio


def one_row_case(L, tab, k, cfg, n, per, seed):
    """Row k of a real table in one launch over random x, eps, keep and ring; then again with x' aliasing x and no model_out."""
    total, scale = n * per, 3.0
    row, kind = tab.table[k].numpy(), tab.kinds[k]
    table = tab.table.cuda()
    x, eps = rnd(seed, total), rnd(seed + 1, (2 if cfg else 1) * total)
    keep, ring = rnd(seed + 2, 3, total) * 10, rnd(seed + 3, 3, total) * 10
    d = Dev(total)
    d.step.fill_(k)
    d.keep[:3 * total], d.ring[:3 * total] = keep.reshape(-1).cuda(), ring.reshape(-1).cuda()
    xd, ed = x.cuda(), eps.cuda()
    launch(L, table, d, xd, ed, n, cfg, scale)
    xt, m, A, am, keep2, ring2 = stage64(row, k, x.numpy(), eps.numpy(), keep.numpy(), ring.numpy(), cfg, scale)
    tag = f"kind {kind} row {k} cfg {cfg} n {n} per {per}"
    ratio = within(d.xp[:total], xt, A, ROUNDS[kind], tag + " x'")
    within(d.out[:total], m, am, ROUNDS_M, tag + " model_out")
    got_keep, got_ring = d.keep[:3 * total].view(3, total).cpu(), d.ring[:3 * total].view(3, total).cpu()
    written_keep = {0: (0, 1), 1: (2,)}.get(kind, ())
    for j in range(3):
        if j in written_keep:
            want = xd.cpu() if j == 0 else d.out[:total].cpu()
            assert torch.equal(got_keep[j], want), f"keep slot {j} of kind {kind}"
        else:
            assert torch.equal(got_keep[j], keep[j]), f"keep slot {j} stays under kind {kind}"
        if kind in (4, 5, 6) and j == k % 3:
            assert torch.equal(got_ring[j], d.out[:total].cpu()), "m goes to ring slot k % 3"
        else:
            assert torch.equal(got_ring[j], ring[j]), f"ring slot {j} stays under kind {kind}"
    assert int(d.step.item()) == k and bool(torch.all(d.ts == SENTINEL)), "advance = 0 moves nothing"
    assert d.guards_intact()
    first = d.xp[:total].clone()
    d.keep[:3 * total], d.ring[:3 * total] = keep.reshape(-1).cuda(), ring.reshape(-1).cuda()
    d.out.fill_(SENTINEL)
    xa = torch.cat([xd, torch.full((8,), SENTINEL, device="cuda")])
    launch(L, table, d, xa, ed, n, cfg, scale, x_prev=xa, out=False)
    assert torch.equal(xa[:total], first), "x' aliasing x, model_out absent: bit for bit the first launch"
    assert guard_ok(xa, total) and bool(torch.all(d.out == SENTINEL)) and d.guards_intact()
    return ratio


@pytest.mark.parametrize("cfg", [0, 1], ids=["plain", "cfg3"])
@pytest.mark.parametrize("method", ["singlestep", "multistep"])
@pytest.mark.parametrize("solver_type", ["dpm_solver", "taylor"])
@pytest.mark.parametrize("x0", [True, False], ids=["x0", "eps"])
def test_every_row_kind(L, tabs, x0, solver_type, method, cfg):
    """Every row of the real table of this (form, solver type, method), at n * per = 1, 255 and 257."""
    tab = tabs[(x0, solver_type, method)]
    want = ([0, 1, 3 if solver_type == "taylor" else 2, 0, 2, 0] if method == "singlestep" else [4, 5, 6, 6, 6, 6]) + [7]
    assert tab.kinds == want
    worst = 0.0
    for k in range(len(tab.kinds)):
        for n, per in ((1, 1), (3, 85), (1, 257)):
            worst = max(worst, one_row_case(L, tab, k, cfg, n, per, seed=400 + 10 * k))
    print(f"  worst ratio: {worst:.3f}")


@pytest.mark.parametrize("key,k", [((True, "taylor", "singlestep"), 2), ((True, "dpm_solver", "multistep"), 3)], ids=["taylor3", "multistep3"])
def test_one_past_a_full_grid(L, tabs, key, k):
    """4096 blocks x 256 threads + 1 element: the grid-stride loop iterates (the two longest chains, under guidance)."""
    one_row_case(L, tabs[key], k, 1, 1, GRID_PASS + 1, seed=520)


def test_a_stage_0_row_never_reads_keep_or_the_ring(L, tabs):
    tab = tabs[(True, "dpm_solver", "singlestep")]
    total, n = 3 * 63, 3
    d = Dev(total)
    d.keep[:3 * total] = float("nan")
    d.ring[:3 * total] = float("nan")
    x, eps = rnd(530, total), rnd(531, total)
    launch(L, tab.table.cuda(), d, x.cuda(), eps.cuda(), n)           # step_idx = 0: row 0, kind 0
    assert bool(torch.isfinite(d.xp[:total]).all()) and bool(torch.isfinite(d.keep[:2 * total]).all())
    assert bool(torch.isnan(d.keep[2 * total:3 * total]).all()) and bool(torch.isnan(d.ring[:3 * total]).all()), "m_s1 and the ring stay"
    zero = np.zeros((3, total), np.float32)
    xt, _, A, _, _, _ = stage64(tab.table[0].numpy(), 0, x.numpy(), eps.numpy(), zero, zero, 0, 1.0)
    within(d.xp[:total], xt, A, ROUNDS[0], "row 0 over keep and ring of NaN")
    # the same for the first multistep row
    tabm = tabs[(False, "taylor", "multistep")]
    d.step.zero_()
    d.keep[:3 * total] = float("nan")
    launch(L, tabm.table.cuda(), d, x.cuda(), eps.cuda(), n)
    assert bool(torch.isfinite(d.xp[:total]).all()) and bool(torch.isnan(d.ring[total:3 * total]).all()) and bool(torch.isnan(d.keep[:3 * total]).all())


def test_a_kind_the_launch_was_not_set_up_for_poisons_x_prime_only(L, tabs):
    tab = tabs[(True, "dpm_solver", "singlestep")]
    total = 257
    d = Dev(total)
    launch(L, tab.table.cuda(), d, rnd(540, total).cuda(), rnd(541, total).cuda(), 1, uses=2)      # row 0 is kind 0, uses names the ring only
    assert bool(torch.isnan(d.xp[:total]).all()) and d.guards_intact()
    assert bool(torch.all(d.keep == SENTINEL)) and bool(torch.all(d.ring == SENTINEL)) and bool(torch.all(d.out == SENTINEL))


@pytest.mark.parametrize("solver_type", ["dpm_solver", "taylor"])
@pytest.mark.parametrize("x0", [True, False], ids=["x0", "eps"])
def test_a_whole_run_chained_through_the_real_table(L, tabs, x0, solver_type):
    """Orders 3, 2, 1 and the denoise row from step_idx = 0 with the advance, n_ts = 5 != n = 3, x' aliasing x.  Every row is compared
    from the kernel's own state before it (latent, keep), so the bound is the one-row bound; the model time written to all n_ts
    entries is the next row's, step_idx goes up by one, and a launch past the end stays on the last row."""
    tab = tabs[(x0, solver_type, "singlestep")]
    n, per, scale = 3, 63, 3.0
    total = n * per
    table = tab.table.cuda()
    d = Dev(total, n_ts=5)
    d.keep[:3 * total] = float("nan")                      # dead contents: row 0 is a stage 0
    x = torch.cat([rnd(550, total).cuda(), torch.full((8,), SENTINEL, device="cuda")])
    ring0 = np.zeros((3, total), np.float32)
    for k, kind in enumerate(tab.kinds):
        eps = rnd(551 + k, 2 * total)
        x_before, keep_before = x[:total].cpu().numpy(), np.nan_to_num(d.keep[:3 * total].view(3, total).cpu().numpy())
        launch(L, table, d, x, eps.cuda(), n, 1, scale, x_prev=x, advance=1, uses=1)
        xt, m, A, am, _, _ = stage64(tab.table[k].numpy(), k, x_before, eps.numpy(), keep_before, ring0, 1, scale)
        within(x[:total], xt, A, ROUNDS[kind], f"row {k} kind {kind} x'")
        within(d.out[:total], m, am, ROUNDS_M, f"row {k} model_out")
        assert int(d.step.item()) == k + 1
        assert d.ts[:5].cpu().tolist() == [tab.table[k, 15].item()] * 5, "all n_ts entries = the model time of the next row"
        assert d.guards_intact() and guard_ok(x, total)
    assert bool(torch.all(d.ring == SENTINEL)), "a singlestep run never touches the ring"
    launch(L, table, d, x, rnd(570, 2 * total).cuda(), n, 1, scale, x_prev=x, advance=1, uses=1)
    assert int(d.step.item()) == len(tab.kinds) and d.guards_intact(), "past the end: the last row again, no index beyond the table"


@pytest.mark.parametrize("cfg", [0, 1], ids=["plain", "cfg3"])
def test_a_thresholded_row_through_predict_quantile_and_stage(L, cfg):
    """The three launches of a thresholded evaluation over a real thresholded table (multistep order 2, row 1): x0_pre against float64,
    s bit for bit the restated quantile of the kernel's own x0_pre (with one sample above max_val and one at it), and the update
    from m = clamp(x0_pre, -s, s) / s."""
    from dsml_thesis_amd.dpm_solver import QUANTILE_P, method_table
    tab = method_table(O.register_schedule(**W.SCHEDULE)["alphas_cumprod"], steps=5, order=2, method="multistep", predict_x0=True,
                       thresholding=True)
    assert all(int(f) == 3 for f in tab.table[:, 14])
    n, per, scale, k = 2, 3073, 3.0, 1
    total = n * per
    table = tab.table.cuda()
    x, eps, ring = rnd(580, total), rnd(581, (2 if cfg else 1) * total), rnd(582, 3, total)
    x[per:] *= 0.01                                        # the second sample's x0 stays below max_val
    eps.view(-1, n, per)[:, 1] *= 0.01
    d = Dev(total)
    d.step.fill_(k)
    d.ring[:3 * total] = ring.reshape(-1).cuda()
    xd, ed = x.cuda(), eps.cuda()
    x0_pre, s = guarded(total), guarded(n)
    stream = torch.cuda.current_stream().cuda_stream
    L.call("ldmk_dpm_predict_x0", xd.data_ptr(), ed.data_ptr(), table.data_ptr(), d.step.data_ptr(), scale, cfg, x0_pre.data_ptr(), per, n,
           table.shape[0], stream)
    row = tab.table[k].numpy().copy()
    plain = row.copy()
    plain[14], plain[2] = 1., 7.                           # the unthresholded data prediction is a kind-7 row's x'
    p64, _, A, _, _, _ = stage64(plain, k, x.numpy(), eps.numpy(), np.zeros((3, total), np.float32), ring.numpy(), cfg, scale)
    torch.cuda.synchronize()
    within(x0_pre[:total], p64, A, ROUNDS_M, "x0_pre")
    max_val = float(np.abs(p64[per:]).max() * 2)
    L.call("ldmk_abs_quantile_rows", x0_pre.data_ptr(), n, per, QUANTILE_P, max_val, s.data_ptr(), stream)
    torch.cuda.synchronize()
    pre = x0_pre[:total].cpu().numpy().reshape(n, per)
    s_ref = abs_quantile_rows_ref(pre, QUANTILE_P, max_val)
    assert np.array_equal(s[:n].cpu().numpy().view(np.uint32), s_ref.view(np.uint32)) and s_ref[0] > np.float32(max_val) == s_ref[1]
    assert bool((np.abs(pre[0]) > s_ref[0]).any()), "clamping changes an element"
    launch(L, table, d, xd, ed, n, cfg, scale, uses=2, x0_pre=x0_pre, s=s)
    xt, m, A, am, _, ring2 = stage64(row, k, x.numpy(), eps.numpy(), np.zeros((3, total), np.float32), ring.numpy(), cfg, scale,
                                     x0_pre=pre.reshape(-1), s=s_ref, per=per)
    assert np.abs(m).max() == 1.0
    within(d.xp[:total], xt, A, ROUNDS[5], "thresholded x'")
    within(d.out[:total], m, am, ROUNDS_M, "thresholded m")
    assert torch.equal(d.ring[:3 * total].view(3, total)[k % 3], d.out[:total]), "the ring holds the thresholded value"
    assert d.guards_intact() and guard_ok(x0_pre, total) and guard_ok(s, n)
