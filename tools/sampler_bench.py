"""PLMS and DPM-Solver against DDIM at bench.py's headline shape (64x64x4 latent, batch 16, class-conditional FR model), in one process.

    python tools/sampler_bench.py [--latent 64] [--batch 16] [--S 50] [--rounds 7] [--out profiles/plms_timing.txt]
    python tools/sampler_bench.py --samplers ddim,dpm --dpm-S 20 --out profiles/dpm_timing.txt

Timed, form by form and alternated round by round (host clock around work that ends in a device synchronise; median and range
of `--rounds` rounds; every graph captured and every shape warmed up before the first timed round):
  step     ms per graphed step: `--S` replays of the captured step of each sampler (UNet program + update + advance).  The PLMS
           graph is the multistep one; its ring is full after three replays, so the window is order-4 steps.  The DPM-Solver graph
           is over the float-time program; replayed past its last step it stays on the last row of its table (order 2 at S >= 15).
  sample   the whole `sample(S, use_graph=True)` call of each sampler: schedule, conditioning, context program, S steps, for
           PLMS the eager first step with its second UNet evaluation.  DPM-Solver runs `--dpm-S` steps (default 20: what
           DPM-Solver++(2M) is used at in place of DDIM's 50) and is reported against DDIM's `--S`.
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
from dsml_thesis_amd.dpm_solver import DPMSolverSampler  # noqa: E402
from dsml_thesis_amd.plms import PLMSSampler  # noqa: E402

KINDS = {"ddim": DDIMSampler, "plms": PLMSSampler, "dpm": DPMSolverSampler}


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
    ap.add_argument("--dpm-S", type=int, default=20)
    ap.add_argument("--samplers", default="ddim,plms", help="comma-separated, of ddim, plms, dpm; ddim is the yardstick")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampler_bench: needs the GPU (a time taken anywhere else says nothing)")
    B, H = a.batch, a.latent
    names = a.samplers.split(",")
    assert names[0] == "ddim" and set(names) <= set(KINDS), names
    steps = {k: (a.dpm_S if k == "dpm" else a.S) for k in names}
    ucfg = synth.NS_UNET if H == 64 else synth.FR_UNET
    m = synth.make_fr_model(gain=0.25, unet=ucfg, vq=synth.VQ_F4_256 if H == 64 else synth.VQ_F4, device="cuda")
    labels = (torch.arange(B, device="cuda") % 8)[:, None]
    c = m.cond_stage_model.embedding(labels)
    shape = [ucfg["in_channels"], H, H]
    torch.manual_seed(0)
    x_T = torch.randn(B, *shape, device="cuda")
    kw = {k: dict(S=steps[k], batch_size=B, shape=shape, conditioning=c, eta=0.0, x_T=x_T, verbose=False, use_graph=True) for k in names}
    samplers = {k: KINDS[k](m) for k in names}
    outs = {k: s.sample(**kw[k])[0] for k, s in samplers.items()}             # captures every graph
    for k, s in samplers.items():
        assert torch.isfinite(outs[k]).all() and torch.equal(s.sample(**kw[k])[0], outs[k]), k
    unet = m.model.diffusion_model
    gen0, denied = unet.generation, len(unet.arithmetic_status()["denied"])      # (the programs below are all of this model state)
    pg = {k: unet.program(B, H, H, 1, 0, float_time=(k == "dpm")) for k in names}
    graphs = {k: next(iter(getattr(pg[k], f"_{k}_loops").values()))["graph"] for k in names}

    def replays(g):
        def run():
            for _ in range(a.S):
                g.replay()
        return run
    step, whole = {k: [] for k in samplers}, {k: [] for k in samplers}
    for k in samplers:
        timed(replays(graphs[k]))                                               # warm: the rings fill, the counters sit at their last index
    for _ in range(a.rounds):
        for k in samplers:
            step[k].append(1e3 * timed(replays(graphs[k])) / a.S)
    # the DDIM graph on the DPM run's data: the launches of the two steps are the same but for the embedding and the update, so a
    # difference per step that survives here is not a launch's (replayed at its last index DDIM leaves the latent where it is)
    cross = []
    if "dpm" in names:
        x_ddim = pg["ddim"].inputs["x"]
        keep = x_ddim.clone()
        x_ddim.copy_(pg["dpm"].inputs["x"])
        timed(replays(graphs["ddim"]))
        for _ in range(a.rounds):
            cross.append(1e3 * timed(replays(graphs["ddim"])) / a.S)
        x_ddim.copy_(keep)
    # replays past the end of a schedule belong to no run: a range flag they raised is dropped here, not charged to the next sample()
    if unet._sites is not None:
        unet._sites.raised()
    if unet._ln_flag is not None:
        unet._ln_flag.zero_()
    for _ in range(a.rounds):
        for k, s in samplers.items():
            whole[k].append(1e3 * timed(lambda: s.sample(**kw[k])))
    replanned = unet.generation != gen0
    fmt = lambda v: f"{statistics.median(v):9.3f}  (min {min(v):.3f}, max {max(v):.3f})"
    med = statistics.median
    why = {"plms": " (one more UNet evaluation: the first step makes two)",
           "dpm": f" ({steps.get('dpm')} steps against {a.S}: one UNet evaluation per step, the first included)"}
    lines = [f"sampler_bench: {H}x{H}x{shape[0]} latent, batch {B}, S = {a.S}, guidance 1, hipGraph steps, {a.rounds} rounds alternated; "
             f"{torch.cuda.get_device_name(0)}; {denied} sites of the model in bf16x3 after a raised range flag"]
    lines += [f"ms per graphed step      {k} {fmt(step[k])}" for k in names]
    lines += [f"  {k} - ddim per step   {med(step[k]) - med(step['ddim']):+.3f} ms" for k in names[1:]]
    if cross:
        lines += [f"ms per graphed step      ddim on the dpm run's latent (|x| up to {pg['dpm'].inputs['x'].abs().max().item():.0f}) {fmt(cross)}"]
    lines += [f"ms per sample(S={steps[k]})     {k} {fmt(whole[k])}" for k in names]
    lines += [f"  {k} - ddim per run    {med(whole[k]) - med(whole['ddim']):+.3f} ms{why[k]}" for k in names[1:]]
    if replanned:
        lines += ["  (a range flag re-planned the model during the sample() rounds: their maxima include a repeated run)"]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
