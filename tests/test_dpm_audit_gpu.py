"""GPU: the recorded-launch-program audit (tests/program_audit.py, the rules of tests/test_program_audit_gpu.py) over the FLOAT-TIME
launch programs -- `UNetModel.program(..., float_time=True)`, whose timestep input is the fp32 `t_f32` embedded by
ldmk_timestep_embedding_f32 -- plain (the plans of a 16-sample job) and small-batch.

  static   R1-R5: lifetimes, releases, kept inputs / outputs, every pointer in a live block, every extent inside its buffer
  dynamic  D1 pooled == unpooled, same launches    D2 0xFF in every workspace byte changes nothing and raises no flag
           D3 inputs A, B, A: the third output is the first
and next to them: the float-time program differs from the integer one in the embedding launch and the input's name alone."""
import pytest
import torch

import program_audit as A
from conftest import rnd
from oracle import weights as W

pytestmark = pytest.mark.gpu


def _inputs(seed, n=2, hw=32):
    return dict(x=rnd(41 + seed, n, 3, hw, hw), t_f32=torch.tensor([[799.2, 0.5], [999.0, 333.25]][seed % 2][:n]),
                context=rnd(42 + seed, n, 512))


@pytest.mark.parametrize("policy", [16, None], ids=["plain", "small-batch"])
def test_float_time_program(policy):
    from test_unet_gpu import make_unet
    m, _ = make_unet(W.FR_UNET)
    m.policy_batch = policy

    def build():
        m._programs.clear()
        pg = m.program(2, 32, 32, 1, 0, float_time=True)
        m._programs.clear()                                # (no audited program stays cached)
        return pg

    def flags():
        st = m.arithmetic_status()
        return set(st["flags_up"]) | ({"<layernorm guard>"} if st["ln_flag_up"] else set())
    a, b = _inputs(0), _inputs(1)
    pooled = build()
    assert bool(getattr(pooled, "small_route", False)) == (policy is None)
    assert "t_f32" in pooled.inputs and "t" not in pooled.inputs and pooled.inputs["t_f32"].dtype == torch.float32
    names = [k[3] for k in pooled.calls]
    assert names.count("ldmk_timestep_embedding_f32") == 1 and "ldmk_timestep_embedding" not in names
    first = A.drive(pooled, a)
    flags0 = flags()
    assert A.finite(first)
    A.poison(pooled)
    poisoned = A.drive(pooled, a)
    assert A.finite(poisoned) and A.same(first, poisoned), "D2: a kernel reads memory that no call of the program wrote"
    assert not (flags() - flags0), "D2: garbage in the workspace raised a flag"
    A.drive(pooled, b)
    assert A.same(first, A.drive(pooled, a)), "D3: the result depends on what the workspace held (A, B, A: third != first)"
    with A.Recorder() as rec:
        unpooled = build()
    rep = A.audit(rec, unpooled)
    print(f"float-time, policy {policy}: {rep.calls} calls, {rep.pointers} pointer arguments checked, {len(rec.buffers)} buffers")
    assert rep.pointers > 0 and not rep.findings, f"static audit: {rep}"
    assert names == [k[3] for k in unpooled.calls] and [k[3] for k in pooled.ctx_program.calls] == [k[3] for k in unpooled.ctx_program.calls]
    assert A.same(first, A.drive(unpooled, a)), "D1: the pool changes the result"
    # the integer program of the same shape: the same launches but for the embedding, and (the key apart) cached side by side
    m._programs.clear()
    pi, pf = m.program(2, 32, 32, 1, 0), m.program(2, 32, 32, 1, 0, float_time=True)
    assert pi is not pf and pi is m.program(2, 32, 32, 1, 0) and pf is m.program(2, 32, 32, 1, 0, float_time=True)
    assert list(pi.inputs) == ["t" if k == "t_f32" else k for k in pf.inputs] and pi.inputs["t"].dtype == torch.int64
    assert [k[3] for k in pi.calls] == ["ldmk_timestep_embedding" if k == "ldmk_timestep_embedding_f32" else k for k in names]
    m._programs.clear()
