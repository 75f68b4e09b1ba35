"""GPU: the last transformer block's ff.net.2 and proj_out folded into ONE pre-split GEMM on two A sources (ops.fold_pout composes
the weight at pack time, csrc/igemm_ps.hip reads [GEGLU output | ff.net.2's residual] from two PS tensors).
  * the folded tail against the unfused tail, both held to a float64 evaluation of the two-step formula: the fold replaces one
    rounding of the intermediate by one rounding of W', so its maximum error may be at most twice the unfused path's;
  * the launch program emit_spatial_transformer builds with LDMK_FOLD_POUT=1 against =0."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import rnd
from oracle import weights as W
from test_ops_gpu import close, ops  # noqa: F401  (the `ops` fixture)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _tail_weights(C, gain=0.25, seed=11):
    keys = {}
    W._spatial_transformer(keys, "", C, C // 32, 32, 1, 512)
    sd = W.synth_state_dict(keys, seed=seed, gain=gain)
    q = "transformer_blocks.0."
    return sd[q + "ff.net.2.weight"], sd[q + "ff.net.2.bias"], sd["proj_out.weight"], sd["proj_out.bias"]


@pytest.mark.parametrize("scale", [1.0, 16.0, 1.0 / 16.0], ids=["wpo_x1", "wpo_x16", "wpo_x1_16"])
@pytest.mark.parametrize("C", [64, 160])
@pytest.mark.parametrize("h2", [True, False], ids=["f16x2", "bf16x3"])
def test_folded_tail_is_as_accurate_as_the_unfused_tail(ops, h2, C, scale):
    """n = 2 samples of 64 tokens.  Weights: the synth recipe at gain 0.25; `scale` multiplies proj_out's weight, which moves the
    magnitude of both halves of W' against the fixed F16X2 activation scale and of the result against its residual.
    Both errors are printed per case; measured on MI355X: profiles/fold_pout_errors.txt (ratios 0.76 - 1.21)."""
    M, hw = 128, 64
    w2, b2, wpo, bpo = _tail_weights(C)
    wpo = wpo * scale
    g, hres, x = rnd(821, M, 4 * C), rnd(822, M, C), rnd(823, M, C)
    ref = x.double() + (hres.double() + g.double() @ w2.double().t() + b2.double()) @ wpo.reshape(C, C).double().t() + bpo.double()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda") if h2 else None
    gps, hps = ops.pack_ps(g.cuda(), h2_flag=flag), ops.pack_ps(hres.cuda(), h2_flag=flag)
    # folded: one GEMM, K = 5 C
    wf, bf = ops.fold_pout(w2.cuda(), b2.cuda(), wpo.cuda(), bpo.cuda())
    assert not h2 or ops.fold_pout_h2_ok(wf, 4 * C)
    out_f = torch.empty(M, C, device="cuda")
    a = ops.make_igemm_args(M, C, 5 * C, None, 5 * C, wf, out_f, C, hw, tile_cfg=27, splitk=1, a_ps=gps, w_ps=ops.pack_wps(wf, h2=h2), bias=bf,
                            residual=x.cuda(), range_flag=flag, a_ps1=hps, a_ps_k0=4 * C)
    ops.igemm(a)
    # unfused: ff.net.2 on its pre-split tile (+ bias + residual), then proj_out as the row GEMM runs it (f32 matrix cores)
    w2p, wpop = ops.pack_linear(w2.cuda()), ops.pack_linear(wpo.cuda())
    hcur = torch.empty(M, C, device="cuda")
    a = ops.make_igemm_args(M, C, 4 * C, None, 4 * C, w2p, hcur, C, hw, tile_cfg=27, splitk=1, a_ps=gps, w_ps=ops.pack_wps(w2p, h2=h2), bias=b2.cuda(),
                            residual=hres.cuda(), range_flag=flag)
    ops.igemm(a)
    out_u = torch.empty(M, C, device="cuda")
    ops.igemm(ops.make_igemm_args(M, C, C, hcur, C, wpop, out_u, C, hw, bias=bpo.cuda(), residual=x.cuda()))
    e_f = (out_f.double().cpu() - ref).abs().max().item()
    e_u = (out_u.double().cpu() - ref).abs().max().item()
    print(f"fold_pout_errors: {'f16x2 ' if h2 else 'bf16x3'} C={C:3d} Wpo x{scale:<6g} max|ref| {ref.abs().max().item():7.3f}  "
          f"folded {e_f:.3e}  unfused {e_u:.3e}  ratio {e_f / e_u:.2f}")
    assert flag is None or flag.item() == 0
    assert e_f <= 2.0 * e_u, (e_f, e_u)


# ---- the launch program ---------------------------------------------------------------------------------------------------------
C_, HEADS, N_, H_, W_ = 64, 2, 2, 8, 8


def _emit(ops, sd, fold, h2, monkeypatch, tmp_path, gn=None):
    """One SpatialTransformer (C = 64, 2 heads, 8 x 8, n = 2) through emit_spatial_transformer with pre-split plans forced for the
    GEGLU projection, ff.net.2 and the folded GEMM; returns (program, output NHWC, GroupNorm coefficient planes of the output)."""
    from dsml_thesis_amd import engine, lib as L, unet as U
    rows = N_ * H_ * W_
    table = {f"{rows},{8 * C_},{C_},{L.A_ROWS},{L.TF_LAYERNORM_FOLDED},{L.EPI_GEGLU},1": [28, 1],
             f"{rows},{C_},{4 * C_},{L.A_ROWS},0,0,1": [27, 1],
             f"{rows},{C_},{5 * C_},{L.A_ROWS},0,0,1": [27, 1]}
    path = tmp_path / "ps_table.json"
    path.write_text(json.dumps(table))
    monkeypatch.setenv("LDMK_PS_H2_TABLE" if h2 else "LDMK_PS_TABLE", str(path))
    monkeypatch.setenv("LDMK_FOLD_POUT", "1" if fold else "0")
    engine.reset_tables()
    try:
        m = U._spatial_transformer(C_, HEADS, 32, 1, 512)
        P = {}
        U.pack_spatial_transformer(P, sd, "", m)
        U.pack_gemm_copies(P)
        pg, ctx_pg = engine.Program("cuda"), engine.Program("cuda")
        if h2:
            pg.h2_flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        nb = engine.NetBuilder(pg, N_)
        x0 = rnd(831, N_, C_, H_, W_).permute(0, 2, 3, 1).contiguous().cuda()
        ctx_in = rnd(832, N_, 512).cuda()
        out = U.emit_spatial_transformer(nb, ctx_pg, P, sd, "", m, x0, H_, W_, 1, ctx_in, 512)
        coef = nb.gn(out, None, H_ * W_, gn[0], gn[1], 1e-5)           # from the records the producer's epilogue attached
        ctx_pg.run()
        pg.run()
        torch.cuda.synchronize()
        assert not h2 or pg.h2_flag.item() == 0
        pg._keep_alive = (P, x0, ctx_in, ctx_pg)
        return pg, out, coef
    finally:
        engine.reset_tables()


@pytest.mark.parametrize("h2", [True, False], ids=["f16x2", "bf16x3"])
def test_folded_program_against_the_unfolded_program(ops, h2, monkeypatch, tmp_path):
    keys = {}
    W._spatial_transformer(keys, "", C_, HEADS, 32, 1, 512)
    sd = {k: v.cuda() for k, v in W.synth_state_dict(keys, seed=9).items()}
    gn = ((1 + 0.2 * rnd(833, C_)).cuda(), (0.2 * rnd(834, C_)).cuda())
    pg0, out0, coef0 = _emit(ops, sd, False, h2, monkeypatch, tmp_path, gn)
    pg1, out1, coef1 = _emit(ops, sd, True, h2, monkeypatch, tmp_path, gn)
    names0, names1 = [c[3] for c in pg0.calls], [c[3] for c in pg1.calls]
    # the unfolded program is the parent commit's, launch by launch (recorded there under the same forced plans)
    recorded = json.load(open(os.path.join(HERE, "test_fold_pout_program_calls.json")))
    assert names0 == recorded["f16x2" if h2 else "bf16x3"]
    # one GEMM fewer, the same launches otherwise; GroupNorm records from the epilogue in both (no statistics pass over the output)
    assert names1.count("ldmk_igemm") == names0.count("ldmk_igemm") - 1
    assert sorted(names1 + ["ldmk_igemm"]) == sorted(names0)
    assert names0.count("ldmk_gn_partial") == 1 == names1.count("ldmk_gn_partial")      # (the block INPUT's statistics pass only)
    g0 = [c[2] for c in pg0.calls if c[3] == "ldmk_igemm"]
    g1 = [c[2] for c in pg1.calls if c[3] == "ldmk_igemm"]
    # hcur -- proj_in's buffer, rewritten in place by attn1.to_out and by ff.net.2 -- is not written a third time
    assert sum(1 for a in g0 if a.out == g0[0].out) == 3 and sum(1 for a in g1 if a.out == g1[0].out) == 2
    assert not any((a.N, a.K) == (C_, 4 * C_) for a in g1) and any((a.N, a.K) == (C_, 4 * C_) for a in g0)
    last = g1[-1]
    assert (last.N, last.K, last.a_ps_k0) == (C_, 5 * C_, 4 * C_) and last.a_ps1 and last.stats_out and last.residual
    assert not any(a.a_ps1 for a in g0)
    close(out1, out0.cpu(), 3e-5, 3e-5)
    close(coef1, coef0.cpu(), 1e-5, 1e-5)
    # proj_out.weight changed in place, packed again: the folded program follows the new weight
    sd["proj_out.weight"].mul_(-0.5)
    pg2, out2, _ = _emit(ops, sd, True, h2, monkeypatch, tmp_path, gn)
    pg3, out3, _ = _emit(ops, sd, False, h2, monkeypatch, tmp_path, gn)
    assert (out2 - out1).abs().max().item() > 1e-2
    close(out2, out3.cpu(), 3e-5, 3e-5)
