"""Patch-wise sampling (`split_input_params`): crops as batch items against the reference's structure, on this repo's kernels.

    python tools/patch_bench.py [--latent 64] [--batch 4] [--ks 32] [--stride 16] [--steps 20]

Latent 64x64x3 with ks 32 / stride 16 is L = 9 crops per item.  Timed (device events, median of 20, every shape warmed up):
  new      unfold kernel -> ONE launch program at batch L*B -> fold kernel, captured in a hipGraph (what a sampler step replays)
  looped   the reference's loop (ddpm.py:914-986): torch Unfold, L program calls at batch B, stack, multiply, torch Fold, divide --
           eager as the reference runs it, and captured in a hipGraph as well
  kernels  ldmk_patch_unfold / ldmk_patch_fold alone, with the bytes they move
  sampler  DDIMSampler.sample(S=steps, use_graph=True) patch-wise, wall time per step (UNet + fold + DDIM update + advance)
The two forms must agree (6e-5, two evaluations of the same crops) before anything is timed."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dsml_thesis_amd import ops, synth  # noqa: E402
from dsml_thesis_amd.ddim import DDIMSampler  # noqa: E402
from dsml_thesis_amd.engine import GraphedProgram  # noqa: E402
from rgemm_bench import timeit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--ks", type=int, default=32)
    ap.add_argument("--stride", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    B, H, ks, st = a.batch, a.latent, a.ks, a.stride
    m = synth.make_fr_model(gain=0.25)
    m.split_input_params = dict(ks=(ks, ks), stride=(st, st), vqf=4, patch_distributed_vq=True, tie_braker=False,
                                clip_min_weight=0.01, clip_max_weight=0.5, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
    unet = m.model.diffusion_model
    torch.manual_seed(0)
    x = torch.randn(B, 3, H, H, device="cuda")
    t = torch.full((B,), 500, device="cuda", dtype=torch.long)
    c = m.cond_stage_model.embedding(torch.arange(B, device="cuda")[:, None] % 7)

    # ---- new: crops as batch items
    pe = m._patched_eval(B, 3, H, H, L_ctx=1)
    L_, g = pe.L, pe.g
    pe.x.copy_(x)
    pe.set_t(t)
    pe.set_cond(c)
    pe.run()
    assert not unet.flags_tripped()
    eps_new = pe.eps.clone()

    # ---- looped: the reference's structure on the same kernels
    pg = unet.program(B, ks, ks, 1, 0)
    pg.inputs["context"].copy_(c.reshape(B, -1))
    pg.inputs["t"].copy_(t)
    pg.ctx_program.run()
    unfold = torch.nn.Unfold(kernel_size=(ks, ks), dilation=1, padding=0, stride=(st, st))
    fold = torch.nn.Fold(output_size=(H, H), kernel_size=(ks, ks), dilation=1, padding=0, stride=(st, st))
    weighting, normalization = g.weight.view(1, 1, ks, ks, L_), g.norm.view(1, 1, H, H)
    out = {}

    def looped():
        z = unfold(x)
        z = z.view((z.shape[0], -1, ks, ks, z.shape[-1]))
        outs = []
        for i in range(L_):
            pg.inputs["x"].copy_(z[:, :, :, :, i])
            pg.run()
            outs.append(pg.outputs["eps"].clone())
        o = torch.stack(outs, axis=-1) * weighting
        out["eps"] = fold(o.view((o.shape[0], -1, o.shape[-1]))) / normalization

    looped()
    d = (out["eps"] - eps_new).abs().max().item()
    print(f"latent {H}x{H}x3, ks {ks}, stride {st}: L = {L_} crops per item, B = {B} -> program batch {L_ * B}")
    print(f"crops as batch vs the loop: max |diff| {d:.3e} (max |eps| {eps_new.abs().max().item():.3f})")
    assert d <= 6e-5 * (1 + eps_new.abs().max().item()), d

    g_new, g_loop = GraphedProgram(pe.run), GraphedProgram(looped)
    rows = []
    for rep in range(3):                                   # the versions alternate inside one process: the spread is visible
        rows.append((timeit(g_new.replay), timeit(looped), timeit(g_loop.replay)))
        print(f"  pass {rep}: new (graph) {rows[-1][0]:9.1f} us   looped (eager) {rows[-1][1]:9.1f} us   looped (graph) {rows[-1][2]:9.1f} us")
    best = [min(r[i] for r in rows) for i in range(3)]
    print(f"eps evaluation, best of 3 medians: new {best[0] / 1e3:.3f} ms, looped eager {best[1] / 1e3:.3f} ms ({best[1] / best[0]:.2f}x), "
          f"looped graph {best[2] / 1e3:.3f} ms ({best[2] / best[0]:.2f}x)")

    # ---- the two kernels alone
    crops, e_crops = pe.pg.inputs["x"], pe.pg.outputs["eps"]
    tu = timeit(lambda: ops.patch_unfold(pe.x, ks, ks, st, st, out=crops))
    tf = timeit(lambda: ops.patch_fold(e_crops, g.weight, g.norm, B, st, st, out=pe.eps))
    bu = 4 * (pe.x.numel() + crops.numel())
    bf = 4 * (e_crops.numel() + pe.eps.numel() + g.norm.numel() + g.weight.numel())
    print(f"ldmk_patch_unfold {tu:7.1f} us ({bu / 1e3:.0f} KB moved, {bu / tu * 1e-3:.1f} GB/s)   "
          f"ldmk_patch_fold {tf:7.1f} us ({bf / 1e3:.0f} KB moved, {bf / tf * 1e-3:.1f} GB/s)")

    # ---- the sampler's graphed step in place
    s = DDIMSampler(m)
    kw = dict(S=a.steps, batch_size=B, shape=[3, H, H], conditioning=c, eta=0.0, x_T=x, verbose=False, use_graph=True)
    s.sample(**kw)                                         # captures
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.sample(**kw)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) / a.steps * 1e3)
    print(f"DDIMSampler.sample patch-wise, S = {a.steps}, use_graph=True: {min(walls):.3f} ms per step (wall, best of 3: "
          + ", ".join(f"{w:.3f}" for w in walls) + ")")


if __name__ == "__main__":
    main()
