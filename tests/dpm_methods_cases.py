"""What the three DPM_Solver test modules share: the recorded runs of tools/make_golden_dpm_methods.py (tests/golden/g27_dpm_methods*.npz)
with the settings that made them, the fp32 restatement of the thresholding quantile, and the float64 restatement of one
`ldmk_dpm_stage` row with its rounding bound.  No test lives here."""
import glob
import os

import numpy as np

from conftest import GOLDEN

# tag -> (keywords of DPMSolverSampler.solver, keywords of DPM_Solver.sample, guidance 3.0?); tools/make_golden_dpm_methods.py RUNS
X0 = dict(predict_x0=True)
THR = dict(predict_x0=True, thresholding=True)
RUNS = {
    "ss3_6": (X0, dict(steps=6, order=3), False),
    "ss3_4": (X0, dict(steps=4, order=3), False),
    "ss3_5": (X0, dict(steps=5, order=3), False),
    "ss2_5": (X0, dict(steps=5, order=2), False),
    "ssf2_6": (X0, dict(steps=6, order=2, method="singlestep_fixed"), False),
    "ss3_6_logSNR": (X0, dict(steps=6, order=3, skip_type="logSNR"), False),
    "ss2_4_quadratic": (X0, dict(steps=4, order=2, skip_type="time_quadratic"), False),
    "eps_ss3_6": ({}, dict(steps=6, order=3), False),
    "eps_ms2_5": ({}, dict(steps=5, order=2, method="multistep"), False),
    "eps_ms3_6": ({}, dict(steps=6, order=3, method="multistep", lower_order_final=False), False),
    "tay_ss3_6": (X0, dict(steps=6, order=3, solver_type="taylor"), False),
    "tay_ss2_4": (X0, dict(steps=4, order=2, solver_type="taylor"), False),
    "tay_ms2_5": (X0, dict(steps=5, order=2, method="multistep", solver_type="taylor"), False),
    "eps_tay_ss3_6": ({}, dict(steps=6, order=3, solver_type="taylor"), False),
    "cfg_ss3_6": (X0, dict(steps=6, order=3), True),
    "thr_ms2_5": (THR, dict(steps=5, order=2, method="multistep"), False),             # (max_val is stored with the run)
    "thr_cfg_ss3_6": (THR, dict(steps=6, order=3), True),
    "dz_ms2_5": (X0, dict(steps=5, order=2, method="multistep", denoise_to_zero=True), False),
    "sub_ss2_4": (X0, dict(steps=4, order=2, t_start=0.6, t_end=0.1), False),
    "split_ss2_4": (X0, dict(steps=4, order=2), False),
}
# the orders of the outer steps, as the issue names them
ORDERS = {"ss3_6": [3, 2, 1], "ss3_4": [3, 1], "ss3_5": [3, 2], "ss2_5": [2, 2, 1], "ssf2_6": [2, 2, 2], "ss3_6_logSNR": [3, 2, 1],
          "ss2_4_quadratic": [2, 2], "eps_ss3_6": [3, 2, 1], "eps_ms2_5": [1, 2, 2, 2, 1], "eps_ms3_6": [1, 2, 3, 3, 3, 3],
          "tay_ss3_6": [3, 2, 1], "tay_ss2_4": [2, 2], "tay_ms2_5": [1, 2, 2, 2, 1], "eps_tay_ss3_6": [3, 2, 1], "cfg_ss3_6": [3, 2, 1],
          "thr_ms2_5": [1, 2, 2, 2, 1], "thr_cfg_ss3_6": [3, 2, 1], "dz_ms2_5": [1, 2, 2, 2, 1], "sub_ss2_4": [2, 2], "split_ss2_4": [2, 2]}


def load_goldens():
    """Every g27_dpm_methods*.npz merged into one dict (the runs are spread over files to keep each under the size limit)."""
    out = {}
    files = sorted(glob.glob(os.path.join(GOLDEN, "g27_dpm_methods*.npz")))
    assert files, "tests/golden/g27_dpm_methods*.npz are missing (tools/make_golden_dpm_methods.py)"
    for f in files:
        out.update(dict(np.load(f)))
    return out


def table_kw(tag, g):
    """The keywords of `method_table` for a recorded run."""
    skw, kw, _ = RUNS[tag]
    return dict(kw, predict_x0=skw.get("predict_x0", False), thresholding=skw.get("thresholding", False))


def solver_kw(tag, g):
    skw = dict(RUNS[tag][0])
    if tag + "_max_val" in g:
        skw["max_val"] = float(g[tag + "_max_val"])
    return skw


def bound(g, tag):
    return max(1.5e-4, 4 * float(g[tag + "_d"]))


# ------------------------------------------------------------------------------------------ the quantile, restated in fp32
def fma32(a, b, c):
    """fl32(a b + c) with ONE rounding, for float32 arrays: the product of two float32 is exact in float64, the float64 sum is made
    with its exact error (TwoSum) and rounded to odd, and a round-to-odd float64 rounds to float32 as the exact value does."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = p + c
        bb = t - p
        err = (p - (t - bb)) + (c - bb)
        even = (np.atleast_1d(t).view(np.uint64) & np.uint64(1)) == 0
        t = np.where((err > 0) & even, np.nextafter(t, np.inf), np.where((err < 0) & even, np.nextafter(t, -np.inf), t))
        return t.astype(np.float32)


def abs_quantile_rows_ref(v, q, floor_val):
    """max(quantile(|v|, q, dim=1), floor_val) for float32 v [rows][per] as torch.quantile forms it on the CPU:
    rank = fl32(q (per - 1)), lo = floor, hi = ceil, w = rank - lo, a and b the order statistics at ranks lo and hi, then torch's lerp,
    whose two branches are each ONE fused multiply-add: w < 0.5 ? fma(w, b - a, a) : fma(-(b - a), 1 - w, b), with b - a and 1 - w
    rounded on their own.  (Rounding the product on its own differs from torch in the last bit about once in a few hundred
    rows.)  A row with a NaN is NaN."""
    v = np.asarray(v, np.float32)
    rows, per = v.shape
    a = np.sort(np.abs(v), axis=1)                         # (NaN sorts last)
    rank = np.float32(q) * np.float32(per - 1)
    lo, hi = np.floor(rank), np.ceil(rank)
    w = np.float32(rank - lo)
    A, B = a[:, int(lo)], a[:, int(hi)]
    with np.errstate(invalid="ignore"):
        d = (B - A).astype(np.float32)
        res = fma32(w, d, A) if w < np.float32(0.5) else fma32(-d, np.float32(1) - w, B)
    res = np.where(np.isnan(v).any(axis=1), np.float32(np.nan), res).astype(np.float32)
    return np.where(np.isnan(res), res, np.maximum(res, np.float32(floor_val))).astype(np.float32)


# ------------------------------------------------------------------------------------------ one ldmk_dpm_stage row in float64
# Roundings on the longest chain from the inputs to x', per kind, under guidance in the x0 form (the longest of all forms):
#   e = e_u + scale (e_c - e_u)      3   (sub, mul, add)
#   m = (x - sigma e) / alpha        3   (mul, sub, div)            -> m carries 6; pred / ring / keep slots are held to 6
#   kind 0, 4:  c_0 m, (c_x x - c_0 m)                                        6 + 2 = 8
#   kind 1, 2:  (m - m_s), [5] (.), (.) + (.)                                 6 + 3 = 9
#   kind 3:     (m - m_s), [6] (.) = D1_1, [7] D1_1, ([8] D1_0 - .), / [11] = D1, c_1 D1, + , - c_2 D2        6 + 8 = 14
#               (through D2: (m - m_s), [6], D1_1 - D1_0, 2 (.) exact, / [11], c_2 (.), last subtraction: 6 + 6 = 12)
#   kind 5:     (m - m1), [5] (.), c_1 (.), + (.)                             6 + 4 = 10
#   kind 6:     the chain of ldmk_dpm_step (tests/test_dpm_ops_gpu.py)        14
#   kind 7:     x' = m                                                        6
# In the eps form m = e (3 roundings) and under thresholding m = clamp(x0_pre) / s (1 rounding from the launch's inputs), so those
# chains are shorter; the same R per kind holds every case.  Bound per element: R * 2^-24 * A, A = the update evaluated in float64
# with every term replaced by its absolute value (differences -> sums of absolute values, |.| / |r2 - r1|).
ROUNDS = {0: 8, 1: 9, 2: 9, 3: 14, 4: 8, 5: 10, 6: 14, 7: 6}
ROUNDS_M = 6
U = 2.0 ** -24


def stage64(row, k, x, eps, keep, ring, cfg, scale, x0_pre=None, s=None, per=None):
    """One row in float64 from the same fp32 inputs -> (x', m, A, A_m, keep', ring').  keep [3][total], ring [3][total]."""
    f = lambda a: np.asarray(a).astype(np.float64)
    total = x.shape[0]
    x, eps, keep, ring, r = f(x), f(eps), f(keep), f(ring), f(row)
    ax = np.abs(x)
    if cfg:
        eu, ec, sc = eps[:total], eps[total:], np.float64(np.float32(scale))
        e, ae = eu + sc * (ec - eu), np.abs(eu) + abs(sc) * (np.abs(ec) + np.abs(eu))
    else:
        e, ae = eps[:total], np.abs(eps[:total])
    al, sg, kind, cx, c0 = r[0], r[1], int(r[2]), r[3], r[4]
    flags = int(r[14])
    if not flags & 1:
        m, am = e, ae
    elif flags & 2 and x0_pre is not None:
        sv = np.repeat(f(s), per)
        m = np.clip(f(x0_pre), -sv, sv) / sv
        am = np.abs(m)
    else:
        m, am = (x - sg * e) / al, (ax + sg * ae) / al
    xs, ms, ms1 = keep
    axs, ams, ams1 = np.abs(xs), np.abs(ms), np.abs(ms1)
    m1, m2 = ring[(k + 2) % 3], ring[(k + 1) % 3]
    keep2, ring2 = keep.copy(), ring.copy()
    if kind in (0, 4):
        xt, A = cx * x - c0 * m, abs(cx) * ax + abs(c0) * am
        if kind == 0:
            keep2[0], keep2[1] = x, m
    elif kind in (1, 2):
        xt = (cx * xs - c0 * ms) + r[5] * (m - ms)
        A = abs(cx) * axs + abs(c0) * ams + abs(r[5]) * (am + ams)
        if kind == 1:
            keep2[2] = m
    elif kind == 3:
        d10, d11 = r[5] * (ms1 - ms), r[6] * (m - ms)
        a10, a11 = abs(r[5]) * (ams1 + ams), abs(r[6]) * (am + ams)
        d1, d2 = (r[8] * d10 - r[7] * d11) / r[11], 2. * (d11 - d10) / r[11]
        a1, a2 = (abs(r[8]) * a10 + abs(r[7]) * a11) / abs(r[11]), 2. * (a11 + a10) / abs(r[11])
        xt = ((cx * xs - c0 * ms) + r[9] * d1) - r[10] * d2
        A = abs(cx) * axs + abs(c0) * ams + abs(r[9]) * a1 + abs(r[10]) * a2
    elif kind == 5:
        xt = (cx * x - c0 * m) + r[9] * (r[5] * (m - m1))
        A = abs(cx) * ax + abs(c0) * am + abs(r[9]) * abs(r[5]) * (am + np.abs(m1))
    elif kind == 6:
        d10, d11 = r[5] * (m - m1), r[6] * (m1 - m2)
        a10, a11 = abs(r[5]) * (am + np.abs(m1)), abs(r[6]) * (np.abs(m1) + np.abs(m2))
        d1, d2 = d10 + r[7] * (d10 - d11), r[8] * (d10 - d11)
        a1, a2 = a10 + abs(r[7]) * (a10 + a11), abs(r[8]) * (a10 + a11)
        xt = ((cx * x - c0 * m) + r[9] * d1) - r[10] * d2
        A = abs(cx) * ax + abs(c0) * am + abs(r[9]) * a1 + abs(r[10]) * a2
    else:
        assert kind == 7, kind
        xt, A = m, am
    if kind in (4, 5, 6):
        ring2[k % 3] = m
    return xt, m, A, am, keep2, ring2
