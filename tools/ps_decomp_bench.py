"""Isolated timing of the GEGLU projection on the pre-split F16X2 tiles as the step runs it (folded LayerNorm, out_ps, no fp32
output) at row counts that fill the chip in whole and in fractional rounds of workgroups: does the time follow M, or the round
count?  Also the long-K rows (ff.net.2 + proj_out, the 320-channel convolution as rows) on the 128x160 tile with split-K over
workgroups (27 sk 2: two launches) and with the K groups inside the workgroup (40).  Operand copies are rotated between launches;
every launch is timed on its own and the median is reported.

    python tools/ps_decomp_bench.py [--cfgs 33,34,35,48] [--reps 30] [--longk 27:1,27:2,40:1]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dsml_thesis_amd import lib as L, ops  # noqa: E402

GEGLU = [(640, 5120, (4096, 3200)), (320, 2560, (16384, 6400)), (160, 1280, (65536, 32768))]      # (K, N, row counts)
LONGK = [(16384, 320, 1600), (16384, 320, 2880), (4096, 640, 2560)]                                  # (M, N, K), rows mode


def median_us(fn, n_rot, reps):
    for i in range(5):
        fn(i % n_rot)
    torch.cuda.synchronize()
    ts = []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i % n_rot)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfgs", default="33")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--longk", default="", help="tile:splitk candidates for the long-K rows, e.g. 27:1,27:2,36:1")
    a = ap.parse_args()
    cfgs = [int(c) for c in a.cfgs.split(",") if c]
    flag = torch.zeros(1, device="cuda", dtype=torch.int32)
    R = 3
    g = torch.Generator(device="cuda").manual_seed(1)
    for K, N, Ms in GEGLU:
        w = (torch.randn(K, N, device="cuda", generator=g) / np.sqrt(K)).contiguous()
        wps = ops.pack_wps(w, h2=True)
        bias, cs = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
        for cfg in cfgs:
            per_row = []
            for M in Ms:
                xps = [ops.pack_ps(torch.randn(M, K, device="cuda", generator=g), h2_flag=flag) for _ in range(R)]
                st = torch.stack([torch.zeros(M, device="cuda"), torch.ones(M, device="cuda")], 1).contiguous()
                o_ps = ops.ps_empty(M, N // 2, h2=True)
                args = [ops.make_igemm_args(M, N, K, None, K, w, None, N // 2, M, tile_cfg=cfg, splitk=1, a_ps=xps[r], w_ps=wps, out_ps=o_ps,
                                            range_flag=flag, bias=bias, epi=L.EPI_GEGLU, tf=L.TF_LAYERNORM_FOLDED, row_stats=st, ln_colsum=cs)
                        for r in range(R)]
                try:
                    med, lo, hi = median_us(lambda r: ops.igemm(args[r]), R, a.reps)
                except L.LdmkError as e:
                    print(f"GEGLU K={K:4d} N={N:5d} M={M:6d} cfg {cfg}: refused ({e})", flush=True)
                    continue
                per_row.append(med / M)
                print(f"GEGLU K={K:4d} N={N:5d} M={M:6d} cfg {cfg}: median {med:7.1f} us (min {lo:7.1f}, max {hi:7.1f}) of {a.reps}; "
                      f"{med / M * 1e3:7.3f} ns per row; {2.0 * M * N * K / med / 1e6:6.1f} TFLOP/s", flush=True)
                del xps, args
            if len(per_row) == 2:
                print(f"      K={K:4d} cfg {cfg}: time per row at the smaller M is {per_row[1] / per_row[0]:.3f} x that at the larger "
                      f"(1.000 = time follows M)", flush=True)
    cands = [tuple(int(v) for v in c.split(":")) for c in a.longk.split(",") if c]
    for M, N, K in (LONGK if cands else []):
        w = (torch.randn(K, N, device="cuda", generator=g) / np.sqrt(K)).contiguous()
        wps = ops.pack_wps(w, h2=True)
        xps = [ops.pack_ps(torch.randn(M, K, device="cuda", generator=g), h2_flag=flag) for _ in range(R)]
        bias, res, out = torch.zeros(N, device="cuda"), torch.randn(M, N, device="cuda", generator=g), torch.empty(M, N, device="cuda")
        ws = torch.empty(2 * M * N, device="cuda")
        for cfg, sk in cands:
            args = [ops.make_igemm_args(M, N, K, None, K, w, out, N, M, tile_cfg=cfg, splitk=sk, splitk_ws=ws if sk > 1 else None, a_ps=xps[r],
                                        w_ps=wps, range_flag=flag, bias=bias, residual=res) for r in range(R)]
            try:
                med, lo, hi = median_us(lambda r: ops.igemm(args[r]), R, a.reps)
            except L.LdmkError as e:
                print(f"rows M={M:6d} N={N:4d} K={K:5d} cfg {cfg} sk {sk}: refused ({e})", flush=True)
                continue
            print(f"rows M={M:6d} N={N:4d} K={K:5d} cfg {cfg} sk {sk}: median {med:7.1f} us (min {lo:7.1f}, max {hi:7.1f}) of {a.reps}; "
                  f"{2.0 * M * N * K / med / 1e6:6.1f} TFLOP/s", flush=True)


if __name__ == "__main__":
    main()
