"""ops.fold_pout: ff.net.2 followed by proj_out composed into ONE Linear on the K-concat [g | h2] (the weights of the two-source
pre-split GEMM that ends a SpatialTransformer).  Pure torch, CPU tensors: no GPU."""
import torch


def _case(C=64, ch=64, M=50, seed=5):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(w2=r(C, 4 * C) / (4 * C) ** 0.5, b2=0.1 * r(C), wpo=r(ch, C, 1, 1) / C ** 0.5, bpo=0.1 * r(ch),
                g=r(M, 4 * C), h2=r(M, C), x=r(M, ch))


def test_fold_pout_is_the_two_step_formula_in_float64():
    from dsml_thesis_amd import ops
    c = _case()
    w, b = ops.fold_pout(c["w2"], c["b2"], c["wpo"], c["bpo"], dtype=torch.float64)
    assert w.shape == (5 * 64, 64) and b.shape == (64,) and w.dtype == torch.float64 and w.is_contiguous()
    wpo = c["wpo"].reshape(64, 64)
    hcur = c["h2"] + c["g"] @ c["w2"].t() + c["b2"]                   # ff.net.2 + residual
    two_step = c["x"] + hcur @ wpo.t() + c["bpo"]                     # proj_out + block residual
    folded = torch.cat([c["g"], c["h2"]], 1) @ w + b + c["x"]
    assert ((folded - two_step).abs().max() / two_step.abs().max()).item() < 1e-12


def test_fold_pout_rounds_once_to_fp32():
    """W' is composed in float64 and rounded ONCE: every fp32 element is within 1 ulp of the float64 product (fp32 inputs, as the
    pack path passes them)."""
    from dsml_thesis_amd import ops
    c = {k: v.float() for k, v in _case(seed=6).items()}
    w, b = ops.fold_pout(c["w2"], c["b2"], c["wpo"], c["bpo"])
    assert w.dtype == torch.float32 and b.dtype == torch.float32
    wpo = c["wpo"].reshape(64, 64).double()
    exact = torch.cat([c["w2"].double().t() @ wpo.t(), wpo.t()], 0)
    ulp = torch.exp2(torch.floor(torch.log2(exact.abs().clamp_min(1e-300))) - 23)
    assert ((w.double() - exact).abs() <= ulp).all()
    assert torch.equal(w[4 * 64:], c["wpo"].reshape(64, 64).t())      # the proj_out half is the weight itself
    be = c["b2"].double() @ wpo.t() + c["bpo"].double()
    assert ((b.double() - be).abs() <= torch.exp2(torch.floor(torch.log2(be.abs().clamp_min(1e-300))) - 23)).all()


def test_fold_pout_f16x2_exponent_rule():
    """One F16X2 exponent serves both halves of W' while the smaller half's largest element is within 2^-16 of the larger's (its lo
    plane stays a normal fp16); beyond that the pack path refuses the F16X2 copy."""
    from dsml_thesis_amd import ops
    w = torch.ones(160, 32)
    w[:128] *= 2.0 ** -10
    assert ops.fold_pout_h2_ok(w, 128)
    w[:128] *= 2.0 ** -10
    assert not ops.fold_pout_h2_ok(w, 128)
    assert not ops.fold_pout_h2_ok(torch.zeros(160, 32), 128)
