"""GPU: the LDS-staged Winograd input transform and the vectorised output transform (csrc/winograd.hip) against the kernels they
replace, which stay in the library as ldmk_winograd_input_ps_v1 / _h2_v1 / ldmk_winograd_output_v1.  The bar is the same bits
everywhere -- the staged kernels apply the same expressions in the same order, only once per pixel and with wider accesses -- so
every comparison is torch.equal, over the whole buffer (the padding rows of a ragged last block included)."""
import itertools

import pytest
import torch

from conftest import rnd
from test_ops_gpu import ops  # noqa: F401  (the `ops` fixture)

pytestmark = pytest.mark.gpu

# (n, c0, c1, h, w)
INPUT_CASES = [
    (2, 64, 0, 8, 8),          # a 32-tile block spans two samples with different coef
    (3, 64, 32, 4, 6),         # tw = 3, 18 tiles, ragged block (dispatched to v1)
    (1, 48, 16, 16, 16),       # the x0 / x1 seam inside a channel block
    (1, 80, 0, 16, 16),        # five k-slabs, partial channel block
    (2, 160, 160, 16, 16),     # the step's own geometry, small
    (1, 320, 0, 32, 32),       # the step's own geometry, small
]
# (n, h, w, cout)
OUTPUT_CASES = [
    (1, 4, 8, 40),             # R = 2, one band
    (2, 8, 8, 64),             # R = 2
    (2, 16, 16, 640),          # 2.5 blocks of 256 channels of v1
    (1, 32, 32, 320),          # two chunks per band
    (1, 16, 16, 6),            # cout % 4 != 0: v1, without records
]


def _flag():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _inputs(case):
    n, c0, c1, h, w = case
    C = c0 + c1
    x0 = rnd(900, n, h, w, c0).cuda()
    x1 = rnd(901, n, h, w, c1).cuda() if c1 else None
    coef = torch.stack([1.0 + 0.2 * rnd(902, n, C), 0.3 * rnd(903, n, C)], 1).contiguous().cuda()
    return x0, x1, coef


def _input_ps(ops, name, case, x0, x1, coef, silu, h2):
    """One launch of an input-transform entry point into a buffer pre-filled with 0xAA; returns (buffer, range flag value)."""
    from dsml_thesis_amd import lib as L
    n, c0, c1, h, w = case
    tiles = n * (h // 2) * (w // 2)
    V = ops.ps_empty(tiles, c0 + c1, batch=16, h2=h2)
    V.fill_(0xAA)
    args = [x0.data_ptr(), c0, 0 if x1 is None else x1.data_ptr(), c1, 0 if coef is None else coef.data_ptr(), 1 if silu else 0, n, h, w,
            V.data_ptr()]
    flag = _flag()
    if h2:
        args.append(flag.data_ptr())
    L.call(name, *args, ops.stream())
    return V, int(flag.item())


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("with_coef", [True, False])
@pytest.mark.parametrize("case", INPUT_CASES)
def test_staged_input_ps_is_bitwise_v1(ops, case, with_coef, silu):
    """PL = 3: the public entry point, the v1 entry point and pack_ps of the fp32 transform."""
    from dsml_thesis_amd import lib as L
    n, c0, c1, h, w = case
    C = c0 + c1
    x0, x1, coef = _inputs(case)
    coef = coef if with_coef else None
    new, _ = _input_ps(ops, "ldmk_winograd_input_ps", case, x0, x1, coef, silu, False)
    old, _ = _input_ps(ops, "ldmk_winograd_input_ps_v1", case, x0, x1, coef, silu, False)
    assert torch.equal(new, old)
    tiles = n * (h // 2) * (w // 2)
    V = torch.empty(16, tiles, C, device="cuda")
    L.call("ldmk_winograd_input", x0.data_ptr(), c0, 0 if x1 is None else x1.data_ptr(), c1, 0 if coef is None else coef.data_ptr(),
           1 if silu else 0, n, h, w, V.data_ptr(), ops.stream())
    ref = ops.pack_ps(V)
    nb = (tiles // 32) * (C // 16) * 3072          # whole row blocks; the ragged block's rows are compared through unpack_ps
    assert torch.equal(new[:, :nb], ref[:, :nb])
    newc, Vc = new.cpu(), V.cpu()
    for p in range(16):
        hi, mid, lo = ops.unpack_ps(newc[p], tiles, C)
        assert torch.equal(hi, Vc[p].to(torch.bfloat16).float())
        assert torch.equal((hi.double() + mid.double() + lo.double()).float(), Vc[p])


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("with_coef", [True, False])
@pytest.mark.parametrize("case", INPUT_CASES)
def test_staged_input_ps_h2_is_bitwise_v1(ops, case, with_coef, silu):
    """PL = 2 (F16X2): the same buffer, and the range flag stays 0 on data below the range."""
    x0, x1, coef = _inputs(case)
    coef = coef if with_coef else None
    new, fnew = _input_ps(ops, "ldmk_winograd_input_ps_h2", case, x0, x1, coef, silu, True)
    old, fold = _input_ps(ops, "ldmk_winograd_input_ps_h2_v1", case, x0, x1, coef, silu, True)
    assert torch.equal(new, old)
    assert fnew == 0 and fold == 0


@pytest.mark.parametrize("case", [(2, 64, 0, 8, 8), (1, 48, 16, 16, 16), (1, 320, 0, 32, 32)])
def test_staged_input_ps_h2_range_flag(ops, case):
    """One input element of 5000 (no scale / shift, no SiLU: nothing else changes) puts V elements of exactly one tile at or
    above 1000: the flag is raised, whether that tile is the first of the launch or the last (last sample, last channel of the
    last source)."""
    n, c0, c1, h, w = case
    x0, x1, _ = _inputs(case)
    for where in ("first", "last"):
        a0, a1 = x0.clone(), None if x1 is None else x1.clone()
        if where == "first":
            a0[0, 0, 0, 3] = 5000.0
        else:
            (a0 if a1 is None else a1)[n - 1, h - 1, w - 1, -1] = 5000.0
        new, fnew = _input_ps(ops, "ldmk_winograd_input_ps_h2", case, a0, a1, None, False, True)
        old, fold = _input_ps(ops, "ldmk_winograd_input_ps_h2_v1", case, a0, a1, None, False, True)
        assert fnew == 1 and fold == 1, where
        assert torch.equal(new, old)


@pytest.mark.parametrize("case", OUTPUT_CASES)
def test_vectorised_output_is_bitwise_v1(ops, case):
    """out and the GroupNorm partial records, with every present / absent combination of bias, per-sample vector, residual and
    records."""
    from dsml_thesis_amd import lib as L
    n, h, w, cout = case
    tiles = n * (h // 2) * (w // 2)
    M = rnd(910, 16, tiles, cout).cuda()
    bias = rnd(911, cout).cuda()
    bvec = rnd(912, n, cout + 8).cuda()[:, :cout]              # a view: the row stride is not the channel count
    res = (3.0 + rnd(913, n, h, w, cout)).cuda()               # mean-dominated results: the records' shift matters
    stats_choices = (False,) if cout % 4 else (False, True)
    for has_bias, has_bvec, has_res, has_stats in itertools.product((False, True), (False, True), (False, True), stats_choices):
        got = []
        for name in ("ldmk_winograd_output", "ldmk_winograd_output_v1"):
            out = torch.full((n, h, w, cout), 7.0, device="cuda")
            rec = torch.full((n * h * w // 32, cout, 3), 7.0, device="cuda")
            L.call(name, M.data_ptr(), bias.data_ptr() if has_bias else 0, bvec.data_ptr() if has_bvec else 0, bvec.stride(0),
                   res.data_ptr() if has_res else 0, out.data_ptr(), rec.data_ptr() if has_stats else 0, n, h, w, cout, ops.stream())
            got.append((out, rec))
        which = (has_bias, has_bvec, has_res, has_stats)
        assert torch.equal(got[0][0], got[1][0]), which
        assert torch.equal(got[0][1], got[1][1]), which
