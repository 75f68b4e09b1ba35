"""GPU: ldmk_diffusion_loss (csrc/objective.hip) against a float64 restatement of ddpm.py:1014-1047 written here.

Bounds.  d = pred - target is one fp32 rounding of fp32 inputs (relative 2^-24, whatever cancels), squares and sums are in double,
and a per-sample weight is formed in double and rounded once; dpred is one more fp32 product.  That is <= 4 * 2^-24 ~ 2.4e-7 on
dpred and on the scalars (sums of non-negative terms); they are held to rtol 1e-6 (x4 margin).  An entry of dlogvar is a sum of
(l_simple_weight / n) (1 - ls_b e^{-lv_b}), which cancels, so it is held to an absolute
1e-6 (l_simple_weight / n) sum_b max(1, ls_b e^{-lv_b}) over the samples that share the entry, and to exactly 0 elsewhere.
Shapes: (1,1,1) is less than one wave, (3,5,7) a ragged 35-pixel tile, (2,16,16) exactly four 64-pixel tiles, (3,64,64) 64
tiles -- the cap of workgroups per sample; c = 3, 4 leave pad lanes, c = 32 none."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T_STEPS = 300            # more than the 256 threads of the final kernel: its strided loop over the dense dlogvar runs twice
LSW, OEW = 0.8, 10.0


@pytest.fixture(scope="module")
def T():
    from dsml_thesis_amd import train_ops
    return train_ops


def _timesteps(kind, n):
    base = {"same": [5, 5, 5], "ends": [0, T_STEPS - 1, 0], "distinct": [11, 257, 140]}[kind]
    return torch.tensor(base[:n], dtype=torch.int64)


def _inputs(n, h, w, c, kind, flip, seed=0):
    rs = np.random.RandomState(1000 * seed + 100 * c + n * h * w)
    hw = h * w
    target = torch.from_numpy(rs.standard_normal((n, c, h, w)).astype(np.float32))
    pred = torch.full((n, hw, 32), float("nan"))                                       # the pad lanes are never read
    pred[..., :c] = torch.from_numpy(rs.standard_normal((n, hw, c)).astype(np.float32))
    same = torch.from_numpy(rs.uniform(size=(n, hw, c)) < 0.15)                        # pred == target there: f'(0) = 0
    if n * hw * c > 1:
        same.view(-1)[0] = True
    pred[..., :c] = torch.where(same, target.view(n, c, hw).permute(0, 2, 1), pred[..., :c])
    t = _timesteps(kind, n)
    logvar = torch.from_numpy(rs.uniform(-1, 1, T_STEPS).astype(np.float32))
    lo, hi = (-8.0, 3.0) if not flip else (3.0, -8.0)
    logvar[t[0]] = lo
    if n > 1 and t[1] != t[0]:
        logvar[t[1]] = hi
    lvlb = torch.from_numpy(rs.uniform(0.0, 0.5, T_STEPS).astype(np.float32))
    lvlb[0] = lvlb[1]
    return pred, target, t, logvar, lvlb, same


def _reference(pred, target, t, logvar, lvlb, loss_type, lsw=LSW, oew=OEW):
    """float64, from the definitions."""
    n, c = target.shape[:2]
    hw = target[0, 0].numel()
    d = pred[..., :c].double() - target.double().view(n, c, hw).permute(0, 2, 1)
    f, fp = (d.abs(), torch.sign(d)) if loss_type == "l1" else (d * d, 2 * d)
    per = c * hw
    ls = f.sum((1, 2)) / per
    lv, w = logvar.double()[t], lvlb.double()[t]
    e = torch.exp(-lv)
    gamma, vlb = (ls * e + lv).mean(), (w * ls).mean()
    dpred = torch.zeros(n, hw, 32, dtype=torch.float64)
    dpred[..., :c] = ((lsw * e + oew * w) / (n * per)).view(n, 1, 1) * fp
    dlogvar, dl_tol = torch.zeros(T_STEPS, dtype=torch.float64), torch.zeros(T_STEPS, dtype=torch.float64)
    for b in range(n):
        dlogvar[t[b]] += lsw / n * (1 - ls[b] * e[b])
        dl_tol[t[b]] += 1e-6 * lsw / n * max(1.0, float(ls[b] * e[b]))
    return dict(scalars=torch.stack([lsw * gamma + oew * vlb, ls.mean(), gamma, vlb]), ls=ls, dpred=dpred, dlogvar=dlogvar, dl_tol=dl_tol)


def _run(T, pred, target, t, logvar, lvlb, loss_type, lsw=LSW, oew=OEW, **kw):
    dpred = torch.full(pred.shape, float("nan"), device="cuda") if kw.get("want_dpred", True) else None
    out = T.diffusion_loss(pred.cuda(), target.cuda(), t.cuda(), logvar.cuda(), lvlb.cuda(), loss_type, lsw, oew, dpred=dpred, **kw)
    torch.cuda.synchronize()
    return out


def _check(out, ref, c):
    print("scalars", out["scalars"].tolist(), "reference", ref["scalars"].tolist())
    torch.testing.assert_close(out["scalars"].double().cpu(), ref["scalars"], rtol=1e-6, atol=0)
    torch.testing.assert_close(out["ls"].double().cpu(), ref["ls"], rtol=1e-6, atol=0)
    dp = out["dpred"].cpu()
    assert bool((dp[..., c:] == 0).all()), "pad lanes of dpred must be exact zeros"
    torch.testing.assert_close(dp.double(), ref["dpred"], rtol=1e-6, atol=0)
    dl = out["dlogvar"].double().cpu()
    hit = ref["dl_tol"] > 0
    assert bool((dl[~hit] == 0).all()), "dlogvar must be exactly zero where no sample sits"
    err = (dl - ref["dlogvar"]).abs()
    print("dlogvar worst error / bound", (err[hit] / ref["dl_tol"][hit]).max().item())
    assert bool((err[hit] <= ref["dl_tol"][hit]).all()), (err[hit], ref["dl_tol"][hit])


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
@pytest.mark.parametrize("c", [3, 4, 32])
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (3, 5, 7), (2, 16, 16), (3, 64, 64)])
def test_objective_against_float64(T, n, h, w, c, loss_type):
    for k, kind in enumerate(("same", "ends", "distinct")):
        pred, target, t, logvar, lvlb, same = _inputs(n, h, w, c, kind, flip=k % 2 == 1, seed=k)
        out = _run(T, pred, target, t, logvar, lvlb, loss_type)
        _check(out, _reference(pred, target, t, logvar, lvlb, loss_type), c)
        if loss_type == "l1":
            assert bool((out["dpred"].cpu()[..., :c][same] == 0).all()), "sign(0) = 0"
        # forward only: the same bits without a dpred; and a second full run is bitwise the first
        fwd = _run(T, pred, target, t, logvar, lvlb, loss_type, want_dpred=False, want_dlogvar=False)
        assert fwd["dpred"] is None and fwd["dlogvar"] is None
        again = _run(T, pred, target, t, logvar, lvlb, loss_type)
        for key in ("scalars", "ls"):
            assert torch.equal(fwd[key], out[key]) and torch.equal(again[key], out[key]), key
        assert torch.equal(again["dpred"], out["dpred"]) and torch.equal(again["dlogvar"], out["dlogvar"])


@pytest.mark.parametrize("loss_type", ["l1", "l2"])
def test_default_weights_reduce_to_the_plain_mean(T, loss_type):
    """l_simple_weight 1, original_elbo_weight 0, logvar 0: loss = loss_simple = loss_gamma, and dpred = f'(d) / (n per)."""
    pred, target, t, _, lvlb, _ = _inputs(2, 16, 16, 3, "distinct", False)
    logvar = torch.zeros(T_STEPS)
    out = _run(T, pred, target, t, logvar, lvlb, loss_type, 1.0, 0.0)
    sc = out["scalars"].cpu()
    assert sc[0] == sc[1] == sc[2]
    _check(out, _reference(pred, target, t, logvar, lvlb, loss_type, 1.0, 0.0), 3)


def test_dlogvar_of_a_batch_is_the_average_of_its_halves(T):
    """The data-parallel identity: two ranks with half the batch each, all-reduced and divided by 2, give the full batch's dlogvar."""
    n, c = 4, 3
    pred, target, _, logvar, lvlb, _ = _inputs(n, 5, 7, c, "same", False)
    t = torch.tensor([5, 9, 5, 9], dtype=torch.int64)                     # both halves hit both entries
    logvar[5], logvar[9] = -8.0, 3.0
    full = _run(T, pred, target, t, logvar, lvlb, "l2")
    halves = [_run(T, pred[s], target[s], t[s], logvar, lvlb, "l2") for s in (slice(0, 2), slice(2, 4))]
    avg = (halves[0]["dlogvar"].double() + halves[1]["dlogvar"].double()) / 2
    ref = _reference(pred, target, t, logvar, lvlb, "l2")
    err = (full["dlogvar"].double() - avg).abs().cpu()
    assert bool((err <= ref["dl_tol"]).all()), (err.max(), ref["dl_tol"].max())
    assert bool((full["dlogvar"].cpu()[ref["dl_tol"] == 0] == 0).all())
    ls_halves = torch.cat([h_["ls"] for h_ in halves])
    assert torch.equal(ls_halves, full["ls"]), "a sample's loss does not depend on the batch around it"


def test_bad_arguments_return_the_library_error_without_launching(T):
    from dsml_thesis_amd import lib as L
    lib = L.load()
    pred, target, t, logvar, lvlb, _ = _inputs(2, 4, 4, 3, "distinct", False)
    dev = [x.cuda() for x in (pred, target, t, logvar, lvlb)]
    dpred = torch.full((2, 16, 32), 7.0, device="cuda")
    dlogvar, scalars, ls = torch.full((T_STEPS,), 7.0, device="cuda"), torch.full((4,), 7.0, device="cuda"), torch.full((2,), 7.0, device="cuda")
    scratch = torch.zeros(lib.ldmk_diffusion_loss_scratch_elems(2), device="cuda", dtype=torch.float64)
    ok = dict(pred=dev[0].data_ptr(), target=dev[1].data_ptr(), t=dev[2].data_ptr(), logvar=dev[3].data_ptr(), lvlb=dev[4].data_ptr(),
              dpred=dpred.data_ptr(), dlogvar=dlogvar.data_ptr(), scalars=scalars.data_ptr(), ls=ls.data_ptr(), n=2, c=3, hw=16,
              T=T_STEPS, loss_type=2, lsw=1.0, oew=0.0, scratch=scratch.data_ptr(), stream=None)
    for bad in (dict(c=33), dict(n=0), dict(n=-2), dict(pred=None), dict(target=None), dict(t=None), dict(logvar=None), dict(lvlb=None),
                dict(scalars=None), dict(ls=None), dict(scratch=None), dict(loss_type=0), dict(pred=ok["pred"] + 4)):
        a = dict(ok, **bad)
        assert lib.ldmk_diffusion_loss(*[a[k] for k in ok]) == -1, bad
        assert b"ldmk_diffusion_loss" in lib.ldmk_last_error()
    torch.cuda.synchronize()
    for buf in (dpred, dlogvar, scalars, ls):
        assert bool((buf == 7.0).all()), "a refused call must not have launched"
    with pytest.raises(L.LdmkError, match="33 channels"):
        T.diffusion_loss(torch.zeros(1, 4, 32, device="cuda"), torch.zeros(1, 33, 2, 2, device="cuda"),
                         torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(10, device="cuda"), torch.zeros(10, device="cuda"))
    with pytest.raises(NotImplementedError, match="unknown loss type"):
        T.diffusion_loss(dev[0], dev[1], dev[2], dev[3], dev[4], "huber")
    a = dict(ok)
    assert lib.ldmk_diffusion_loss(*[a[k] for k in ok]) == 0                          # and the good call goes through
    torch.cuda.synchronize()
    assert bool((dpred[..., 3:] == 0).all()) and bool(torch.isfinite(scalars).all())
