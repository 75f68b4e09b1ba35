"""Winograd F(2x2,3x3) against the direct implicit-GEMM convolution on the UNet's ResBlock shapes (HIP events, median).

    python tools/winograd_bench.py [--latent 64] [--batch 16]
    python tools/winograd_bench.py --transforms      the two transforms alone, staged / vectorised kernel against v1, per shape"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dsml_thesis_amd import lib as L  # noqa: E402
from dsml_thesis_amd import ops  # noqa: E402
from rgemm_bench import timeit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--upsample", action="store_true")
    ap.add_argument("--transforms", action="store_true")
    a = ap.parse_args()
    if a.upsample:
        return upsample_main(a)
    if a.transforms:
        return transforms_main(a)
    n = a.batch
    for lvl, cin, cout in ((2, 640, 640), (2, 1280, 640), (2, 960, 640), (1, 320, 320), (1, 640, 320), (0, 160, 160)):
        h = a.latent >> lvl
        x = torch.randn(n, h, h, cin, device="cuda")
        w = torch.randn(cout, cin, 3, 3, device="cuda") / (9 * cin) ** 0.5
        b = torch.randn(cout, device="cuda")
        res = torch.randn(n, h, h, cout, device="cuda")
        coef = torch.ones(n, 2, cin, device="cuda")
        part = torch.zeros(n * h * h // 32, cout, 3, device="cuda")
        wp, u = ops.pack_conv3x3(w), ops.pack_winograd(w)
        xa = torch.empty_like(x)
        out = torch.empty(n, h, h, cout, device="cuda")
        tiles = n * (h // 2) * (h // 2)
        scratch = (torch.empty(16, tiles, cin, device="cuda"), torch.empty(16, tiles, cout, device="cuda"))

        def direct():
            L.call("ldmk_gn_apply", x.data_ptr(), cin, 0, 0, coef.data_ptr(), xa.data_ptr(), n, h * h, 1, ops.stream())
            ops.conv3x3(xa, wp, b, residual=res, out=out)

        def wino():
            ops.conv3x3_winograd(x, u, b, coef=coef, residual=res, out=out, stats_out=part, scratch=scratch)

        td, tw = timeit(direct), timeit(wino)
        gf = 2.0 * n * h * h * cout * 9 * cin * 1e-9
        print(f"{cin:5d}->{cout:4d} @{h:2d}x{h:<2d} n={n}: gn_apply + direct {td:7.1f} us ({gf / td * 1e3:6.1f} TF)   winograd {tw:7.1f} us "
              f"({gf / tw * 1e3:6.1f} TF direct-equivalent)  x{td / tw:.2f}", flush=True)


def upsample_main(a):
    n = a.batch
    for lvl, c in ((2, 640), (1, 320)):
        h = a.latent >> lvl
        x = torch.randn(n, h, h, c, device="cuda")
        w = torch.randn(c, c, 3, 3, device="cuda") / (9 * c) ** 0.5
        b = torch.randn(c, device="cuda")
        wp, w4 = ops.pack_conv3x3(w), ops.pack_upconv(w)
        out = torch.empty(n, 2 * h, 2 * h, c, device="cuda")
        part = torch.zeros(n * 4 * h * h // 32, c, 3, device="cuda")
        pix = n * h * h
        scratch = (torch.empty(4, pix, 4 * c, device="cuda"), torch.empty(4, pix, c, device="cuda"))
        td = timeit(lambda: ops.conv3x3(x, wp, b, upsample=True, out=out))
        tp = timeit(lambda: ops.upsample_conv3x3_phases(x, w4, b, out=out, stats_out=part, scratch=scratch))
        gf = 2.0 * n * 4 * h * h * c * 9 * c * 1e-9
        print(f"upsample {c}->{c} {h}x{h}->{2 * h}x{2 * h} n={n}: folded-gather conv {td:7.1f} us ({gf / td * 1e3:6.1f} TF)   four 2x2-tap phases "
              f"{tp:7.1f} us ({gf / tp * 1e3:6.1f} TF direct-equivalent)  x{td / tp:.2f}", flush=True)


def transforms_main(a):
    """The F16X2 input transform and the output transform alone on the step's shapes: public entry point (LDS-staged / vectorised
    kernel where the dispatch takes it) against the _v1 entry point, with ldmk_gn_apply_ps_h2 on the same input as the yardstick of
    an elementwise pass into the same layout.  Four buffer sets are rotated so a call does not find its own last output in the
    caches; bytes are the ones the algorithm needs (input read once, outputs written once)."""
    n, sets = a.batch, 4
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")

    def rate(nbytes, us):
        return nbytes / us * 1e-6          # TB/s

    def rotate(calls):
        def run():
            for c in calls:
                c()
        return timeit(run, iters=15, warm=2) / len(calls)

    print(f"input transform (F16X2 PS layout), n={n}: us per launch, TB/s of (x read once + V written)", flush=True)
    for lvl, c0, c1 in ((2, 640, 0), (2, 640, 320), (2, 640, 640), (2, 1280, 640), (1, 320, 0), (1, 320, 320), (1, 640, 320), (3, 1280, 0),
                        (3, 1280, 1280)):
        h = a.latent >> lvl
        C, tiles = c0 + c1, n * (h // 2) * (h // 2)
        x0 = [torch.randn(n, h, h, c0, device="cuda") for _ in range(sets)]
        x1 = [torch.randn(n, h, h, c1, device="cuda") if c1 else None for _ in range(sets)]
        coef = torch.ones(n, 2, C, device="cuda")
        V = [ops.ps_empty(tiles, C, batch=16, h2=True) for _ in range(sets)]
        Y = [ops.ps_empty(n * h * h, C, h2=True) for _ in range(sets)]
        p1 = [0 if t is None else t.data_ptr() for t in x1]
        ts = {}
        for name in ("ldmk_winograd_input_ps_h2", "ldmk_winograd_input_ps_h2_v1"):
            ts[name] = rotate([lambda i=i, name=name: L.call(name, x0[i].data_ptr(), c0, p1[i], c1, coef.data_ptr(), 1, n, h, h, V[i].data_ptr(),
                                                             flag.data_ptr(), ops.stream()) for i in range(sets)])
        tg = rotate([lambda i=i: L.call("ldmk_gn_apply_ps_h2", x0[i].data_ptr(), c0, p1[i], c1, coef.data_ptr(), Y[i].data_ptr(), n, h * h, 1,
                                        flag.data_ptr(), ops.stream()) for i in range(sets)])
        bx, bv, by = n * h * h * C * 4, V[0].numel(), Y[0].numel()
        tn, to = ts["ldmk_winograd_input_ps_h2"], ts["ldmk_winograd_input_ps_h2_v1"]
        route = L.load().ldmk_winograd_input_ps_route(n, h, h, c0, c1)
        print(f"  {c0:4d}+{c1:<4d} @{h:2d}x{h:<2d} route {route}: {tn:6.1f} us {rate(bx + bv, tn):5.2f} TB/s   v1 {to:6.1f} us {rate(bx + bv, to):5.2f} TB/s"
              f"  x{to / tn:.2f}   gn_apply_ps_h2 {tg:6.1f} us {rate(bx + by, tg):5.2f} TB/s", flush=True)
    print(f"output transform (bias + per-sample vector + residual + records), n={n}: TB/s of (M + residual read, out written)", flush=True)
    for lvl, cout in ((2, 640), (1, 320), (1, 640), (3, 1280)):
        h = a.latent >> lvl
        tiles = n * (h // 2) * (h // 2)
        M = [torch.randn(16, tiles, cout, device="cuda") for _ in range(sets)]
        res = [torch.randn(n, h, h, cout, device="cuda") for _ in range(sets)]
        out = [torch.empty(n, h, h, cout, device="cuda") for _ in range(sets)]
        b, bv = torch.randn(cout, device="cuda"), torch.randn(n, cout, device="cuda")
        part = torch.zeros(n * h * h // 32, cout, 3, device="cuda")
        ts = {}
        for name in ("ldmk_winograd_output", "ldmk_winograd_output_v1"):
            ts[name] = rotate([lambda i=i, name=name: L.call(name, M[i].data_ptr(), b.data_ptr(), bv.data_ptr(), cout, res[i].data_ptr(),
                                                             out[i].data_ptr(), part.data_ptr(), n, h, h, cout, ops.stream()) for i in range(sets)])
        nbytes = M[0].numel() * 4 + 2 * out[0].numel() * 4
        tn, to = ts["ldmk_winograd_output"], ts["ldmk_winograd_output_v1"]
        route = L.load().ldmk_winograd_output_route(n, h, h, cout, 1)
        print(f"  ->{cout:4d} @{h:2d}x{h:<2d} route {route}: {tn:6.1f} us {rate(nbytes, tn):5.2f} TB/s   v1 {to:6.1f} us {rate(nbytes, to):5.2f} TB/s  x{to / tn:.2f}",
              flush=True)


if __name__ == "__main__":
    main()
