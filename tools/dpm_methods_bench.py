"""The DPM_Solver loops against the multistep step of DPMSolverSampler at bench.py's headline shape (64x64x4 latent, batch 16,
class-conditional FR model), graphed, in one process.

    python tools/dpm_methods_bench.py [--latent 64] [--batch 16] [--rounds 7] [--out profiles/dpm_methods_timing.txt]

Timed, alternated round by round (host clock around work that ends in a device synchronise; median and range of `--rounds` rounds;
every graph captured and every shape warmed up before the first timed round):
  ms per model evaluation of a whole graphed `sample()` call, divided by its number of evaluations:
    base A, base B   DPMSolverSampler.sample(S=18): multistep DPM-Solver++ order 2, twice -- the spread of the yardstick
    singlestep 3     solver(predict_x0=True).sample(steps=18, order=3): six outer steps of three stages
    thresholded      solver(predict_x0=True, thresholding=True).sample(steps=18, order=2, method='multistep'): two more launches per
                     evaluation (predict x0, quantile)
  us per launch of ldmk_abs_quantile_rows alone at rows = batch, per = latent^2 * 4, and of the ldmk_dpm_stage launch it precedes
    (device events around 200 back-to-back launches).
Nothing is asserted: the numbers are recorded."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsml_thesis_amd import lib as L  # noqa: E402
from dsml_thesis_amd import synth  # noqa: E402
from dsml_thesis_amd.dpm_solver import QUANTILE_P, DPMSolverSampler, method_table  # noqa: E402

NFE = 18


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def launches_us(fn, n=200):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dpm_methods_bench: needs the GPU (a time taken anywhere else says nothing)")
    B, H = a.batch, a.latent
    ucfg = synth.NS_UNET if H == 64 else synth.FR_UNET
    m = synth.make_fr_model(gain=0.25, unet=ucfg, vq=synth.VQ_F4_256 if H == 64 else synth.VQ_F4, device="cuda")
    c = m.cond_stage_model.embedding((torch.arange(B, device="cuda") % 8)[:, None])
    shape = [ucfg["in_channels"], H, H]
    torch.manual_seed(0)
    x_T = torch.randn(B, *shape, device="cuda")
    s = DPMSolverSampler(m)
    single = s.solver(conditioning=c, predict_x0=True, use_graph=True)
    thr = s.solver(conditioning=c, predict_x0=True, thresholding=True, use_graph=True)
    legs = {
        "base A": lambda: s.sample(S=NFE, batch_size=B, shape=shape, conditioning=c, x_T=x_T, use_graph=True)[0],
        "singlestep 3": lambda: single.sample(x_T, steps=NFE, order=3),
        "thresholded": lambda: thr.sample(x_T, steps=NFE, order=2, method="multistep"),
        "base B": lambda: s.sample(S=NFE, batch_size=B, shape=shape, conditioning=c, x_T=x_T, use_graph=True)[0],
    }
    for k, fn in legs.items():                             # captures every graph; a second call replays it
        out = fn()
        assert torch.isfinite(out).all() and torch.equal(fn(), out), k
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            ms[k].append(1e3 * timed(fn) / NFE)
    # the two small launches on their own
    per = shape[0] * H * H
    stream = torch.cuda.current_stream().cuda_stream
    v, s_out = torch.randn(B, per, device="cuda") * 3, torch.empty(B, device="cuda")
    q_us = launches_us(lambda: L.call("ldmk_abs_quantile_rows", v.data_ptr(), B, per, QUANTILE_P, 1.0, s_out.data_ptr(), stream))
    tab = method_table(s.alphas_cumprod, steps=NFE, order=2, method="multistep", predict_x0=True, thresholding=True)
    table, step_idx = tab.table.cuda(), torch.ones(1, dtype=torch.int32, device="cuda")
    x, eps, pre = torch.randn(B, per, device="cuda"), torch.randn(B, per, device="cuda"), torch.randn(B, per, device="cuda")
    ring = torch.zeros(3, B, per, device="cuda")
    u_us = launches_us(lambda: L.call("ldmk_dpm_stage", x.data_ptr(), eps.data_ptr(), table.data_ptr(), step_idx.data_ptr(), 1.0, 0,
                                      pre.data_ptr(), s_out.data_ptr(), 0, ring.data_ptr(), x.data_ptr(), 0, per, B, 0, 0, 0, NFE, 2, stream))
    p_us = launches_us(lambda: L.call("ldmk_dpm_predict_x0", x.data_ptr(), eps.data_ptr(), table.data_ptr(), step_idx.data_ptr(), 1.0, 0,
                                      pre.data_ptr(), per, B, NFE, stream))
    med = statistics.median
    fmt = lambda v_: f"{med(v_):9.3f}  (min {min(v_):.3f}, max {max(v_):.3f})"
    base = med(ms["base A"] + ms["base B"])
    lines = [f"dpm_methods_bench: {H}x{H}x{shape[0]} latent, batch {B}, {NFE} model evaluations per run, guidance 1, hipGraph, {a.rounds} rounds "
             f"alternated; {torch.cuda.get_device_name(0)}"]
    lines += [f"ms per model evaluation  {k:13s} {fmt(ms[k])}" for k in legs]
    lines += [f"  base B - base A         {med(ms['base B']) - med(ms['base A']):+.3f} ms (the yardstick's own spread)"]
    lines += [f"  {k} - base    {med(ms[k]) - base:+.3f} ms" for k in ("singlestep 3", "thresholded")]
    lines += [f"us per launch alone      ldmk_abs_quantile_rows rows {B} per {per}: {q_us:.1f};  ldmk_dpm_stage (thresholded multistep order 2): "
              f"{u_us:.1f};  ldmk_dpm_predict_x0: {p_us:.1f}"]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
