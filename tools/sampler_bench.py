"""PLMS against DDIM at bench.py's headline shape (64x64x4 latent, batch 16, class-conditional FR model), in one process.

    python tools/sampler_bench.py [--latent 64] [--batch 16] [--S 50] [--rounds 7] [--out profiles/plms_timing.txt]

Timed, form by form and alternated round by round (host clock around work that ends in a device synchronise; median and range
of `--rounds` rounds; every graph captured and every shape warmed up before the first timed round):
  step     ms per graphed step: `--S` replays of the captured step of each sampler (UNet program + update + advance).  The PLMS
           graph is the multistep one; its ring is full after three replays, so the window is order-4 steps.
  sample   the whole `sample(S, use_graph=True)` call of each sampler: schedule, conditioning, context program, S steps, for
           PLMS the eager first step with its second UNet evaluation.
Nothing is asserted: the numbers are recorded."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsml_thesis_amd import synth  # noqa: E402
from dsml_thesis_amd.ddim import DDIMSampler  # noqa: E402
from dsml_thesis_amd.plms import PLMSSampler  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--S", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampler_bench: needs the GPU (a time taken anywhere else says nothing)")
    B, H, S = a.batch, a.latent, a.S
    ucfg = synth.NS_UNET if H == 64 else synth.FR_UNET
    m = synth.make_fr_model(gain=0.25, unet=ucfg, vq=synth.VQ_F4_256 if H == 64 else synth.VQ_F4, device="cuda")
    labels = (torch.arange(B, device="cuda") % 8)[:, None]
    c = m.cond_stage_model.embedding(labels)
    shape = [ucfg["in_channels"], H, H]
    torch.manual_seed(0)
    x_T = torch.randn(B, *shape, device="cuda")
    kw = dict(S=S, batch_size=B, shape=shape, conditioning=c, eta=0.0, x_T=x_T, verbose=False, use_graph=True)
    samplers = {"ddim": DDIMSampler(m), "plms": PLMSSampler(m)}
    outs = {k: s.sample(**kw)[0] for k, s in samplers.items()}                # captures both graphs
    for k, s in samplers.items():
        assert torch.isfinite(outs[k]).all() and torch.equal(s.sample(**kw)[0], outs[k]), k
    pg = m.model.diffusion_model.program(B, H, H, 1, 0)
    graphs = {"ddim": next(iter(pg._ddim_loops.values()))["graph"], "plms": next(iter(pg._plms_loops.values()))["graph"]}

    def replays(g):
        def run():
            for _ in range(S):
                g.replay()
        return run
    step, whole = {k: [] for k in samplers}, {k: [] for k in samplers}
    for k in samplers:
        timed(replays(graphs[k]))                                               # warm: the PLMS ring fills, both counters sit at index 0
    for _ in range(a.rounds):
        for k in samplers:
            step[k].append(1e3 * timed(replays(graphs[k])) / S)
    for _ in range(a.rounds):
        for k, s in samplers.items():
            whole[k].append(1e3 * timed(lambda: s.sample(**kw)))
    fmt = lambda v: f"{statistics.median(v):9.3f}  (min {min(v):.3f}, max {max(v):.3f})"
    lines = [f"sampler_bench: {H}x{H}x{shape[0]} latent, batch {B}, S = {S}, guidance 1, hipGraph steps, {a.rounds} rounds alternated; "
             f"{torch.cuda.get_device_name(0)}",
             f"ms per graphed step      ddim {fmt(step['ddim'])}",
             f"ms per graphed step      plms {fmt(step['plms'])}",
             f"  plms - ddim per step   {statistics.median(step['plms']) - statistics.median(step['ddim']):+.3f} ms",
             f"ms per sample(S={S})     ddim {fmt(whole['ddim'])}",
             f"ms per sample(S={S})     plms {fmt(whole['plms'])}",
             f"  plms - ddim per run    {statistics.median(whole['plms']) - statistics.median(whole['ddim']):+.3f} ms "
             f"(one more UNet evaluation: the first step makes two)"]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
