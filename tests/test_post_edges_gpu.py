"""GPU: the branches of ldmk_post (csrc/post.hip) that the small-batch tests do not reach -- the single-launch GroupNorm past
its 15360-value LDS cache (the three reload arms), the row-tiled GroupNorm with a ragged last tile / a tail in the 8-lane tile
walk / the 64 KiB tile / the concat seam, raw_out of a plain source, the LayerNorm templates <8> and <5> at jn = 4, N = 4 --
on ordinary data and on the mean-dominated data of tests/norm_models.py.

Slabs are plain random tensors and their float64 sum is the reference.  raw_out: 1e-4 / 1e-4 like the other ldmk_post tests;
norm_out: the derived bound of norm_models.gn_out_bound / ln_out_bound against float64 of the tensor actually stored."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import norm_models as nm
from conftest import rnd
from norm_models import normcond_line  # noqa: F401  (autouse: one NORMCOND line per test id)
from test_small_batch_gpu import close, ops  # noqa: F401  (the `ops` fixture)

pytestmark = pytest.mark.gpu


def _report(request, what, err, used):
    nm.note(request, f"{what}: max error {err:.3e}, {used:.3f} of its bound")


def _gn_data(data, n, hw, N, c1, nslab, epilogue):
    """-> slabs [nslab][M][N], x1 [M][c1] or None, bias / vec / res or None"""
    M, Cc = n * hw, N + c1
    if data == "mean":
        base = nm.gn_input(800, n, hw, Cc).reshape(M, Cc)
    else:
        base = (rnd(800, M, Cc) * 1.3 + 0.4)
    slabs = torch.stack([base[:, :N].contiguous()] + [0.3 * rnd(801 + k, M, N) for k in range(1, nslab)])
    x1 = base[:, N:].contiguous() if c1 else None
    if not epilogue:
        return slabs, x1, None, None, None
    return slabs, x1, 0.1 * rnd(810, N), rnd(811, n, N), rnd(812, M, N)


def _run_gn(ops, request, n, hw, N, c1, nslab, epilogue, raw, data, eps=1e-5):
    from dsml_thesis_amd import lib as L
    M, Cc = n * hw, N + c1
    slabs, x1, b, vec, res = _gn_data(data, n, hw, N, c1, nslab, epilogue)
    gamma, beta = nm.affine(820, Cc)
    raw_ref = slabs.double().sum(0)
    if epilogue:
        raw_ref = raw_ref + b.double() + vec.double().repeat_interleave(hw, 0) + res.double()
    sentinel = -12345.0
    dev = [None if t is None else t.cuda() for t in (slabs, x1, b, vec, res, gamma, beta)]
    outs = []
    for _ in range(2):
        rawd = torch.full((M, N), sentinel, device="cuda") if raw else None
        out = torch.full((M, Cc), sentinel, device="cuda")
        a = ops.make_post_args(dev[0], M, N, hw, nslab=nslab, bias=dev[2], batch_vec=dev[3], batch_vec_ld=N, residual=dev[4], raw_out=rawd,
                               norm=L.POST_GROUPNORM, x1=dev[1], c1=c1, gamma=dev[5], beta=dev[6], eps=eps, norm_out=out)
        ops.post(a)
        outs.append((rawd, out))
    (rawd, out), (raw2, out2) = outs
    assert torch.equal(out, out2) and (not raw or torch.equal(rawd, raw2)), "fixed summation order: bitwise reproducible"
    if raw:
        close(rawd, raw_ref.float(), 1e-4, 1e-4)
        if not epilogue and nslab == 1:
            assert torch.equal(rawd.cpu(), slabs[0]), "raw_out of a plain source is the source"
        stored = rawd.cpu()
    else:
        stored = slabs[0]                                     # (no raw_out: a plain source, normalised as it is)
    cat = (stored if x1 is None else torch.cat([stored, x1], 1)).reshape(n, hw, Cc)
    y64, mean, rstd = nm.gn_ref(cat, 32, gamma, beta, eps)
    err = (out.cpu().double().reshape(n, hw, Cc) - y64).abs()
    used = (err / nm.gn_out_bound(cat, mean, rstd, gamma, y64)).max().item()
    _report(request, f"norm_out ({data}, {'with' if raw else 'no'} raw_out)", err.max().item(), used)
    assert used <= 1.0, f"norm_out uses {used:.3f} of its bound (max error {err.max().item():.3e})"


DATA = ["plain", "mean"]


# ---- single-launch GroupNorm: 248 rows x 64 channels per group = 15872 values against a cache of 15360 ------------------------------
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("form", ["reload_raw_out", "reload_src", "reload_x1", "exactly_the_cache"])
def test_post_groupnorm_single_launch_past_its_cache(ops, request, form, data):
    if form == "reload_raw_out":        # pending source: the values past the cache are read back from raw_out
        _run_gn(ops, request, 1, 248, 2048, 0, nslab=2, epilogue=True, raw=True, data=data)
    elif form == "reload_src":          # plain source, no raw_out: read again from src
        _run_gn(ops, request, 1, 248, 2048, 0, nslab=1, epilogue=False, raw=False, data=data)
    elif form == "reload_x1":           # groups 16..31 lie in x1: read again from x1
        _run_gn(ops, request, 1, 248, 1024, 1024, nslab=1, epilogue=False, raw=False, data=data)
    else:                               # 240 x 64 = 15360: the last value that still fits
        _run_gn(ops, request, 1, 240, 2048, 0, nslab=2, epilogue=True, raw=True, data=data)


def test_post_groupnorm_past_its_cache_needs_somewhere_to_reload_from(ops):
    from dsml_thesis_amd import lib as L
    M, N = 248, 2048
    slabs, g = torch.zeros(2, M, N, device="cuda"), torch.ones(N, device="cuda")
    out = torch.empty(M, N, device="cuda")
    with pytest.raises(L.LdmkError, match="need raw_out"):
        ops.post(ops.make_post_args(slabs, M, N, M, nslab=2, norm=L.POST_GROUPNORM, gamma=g, beta=g, norm_out=out))


# ---- row-tiled GroupNorm (rows_per_sample >= 512): two launches -------------------------------------------------------------------------
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("nslab", [1, 3])
@pytest.mark.parametrize("shape", [(2, 516, 160, 0),         # 65 tiles (a tail in the 8-lane walk over 64), the last of 4 rows
                                   (1, 516, 1024, 1024),    # C = 2048: a 64 KiB tile
                                   (1, 512, 320, 160)],     # the seam: 15 channels per group
                         ids=nm.case_id)
def test_post_groupnorm_row_tiled_edges(ops, request, shape, nslab, data):
    n, hw, N, c1 = shape
    _run_gn(ops, request, n, hw, N, c1, nslab=nslab, epilogue=True, raw=True, data=data)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("shape", [(2, 516, 160, 0), (1, 512, 320, 160)], ids=nm.case_id)
def test_post_groupnorm_row_tiled_writes_raw_out_of_a_plain_source(ops, request, shape, data):
    """include/ldmk.h: raw_out is optional and written when given -- also when the source is one plain slab with no epilogue
    terms, where the apply launch could read the source itself."""
    n, hw, N, c1 = shape
    _run_gn(ops, request, n, hw, N, c1, nslab=1, epilogue=False, raw=True, data=data)
    _run_gn(ops, request, n, hw, N, c1, nslab=1, epilogue=False, raw=False, data=data)


def test_post_groupnorm_row_tiled_refusals(ops):
    from dsml_thesis_amd import lib as L
    M = 512
    x, g = torch.zeros(M, 2052, device="cuda"), torch.ones(2052, device="cuda")
    out = torch.empty(M, 2052, device="cuda")
    with pytest.raises(L.LdmkError, match="32 groups"):
        ops.post(ops.make_post_args(x, M, 160, M, norm=L.POST_GROUPNORM, gamma=g, beta=g, norm_out=out, groups=16))
    # C = 2052 is not a multiple of 32 groups: the general GroupNorm check refuses it before the row-tiled branch is reached.  (The
    # row-tiled form's own 64 KiB tile limit, C <= 2048, cannot be hit with 32 groups: 64 channels per group already cap C at 2048.)
    with pytest.raises(L.LdmkError, match="C=2052"):
        ops.post(ops.make_post_args(x, M, 2052, M, norm=L.POST_GROUPNORM, gamma=g, beta=g, norm_out=out))
    a = ops.make_post_args(x, M, 160, M, norm=L.POST_GROUPNORM, gamma=g, beta=g, norm_out=out)
    need = L.load().ldmk_post_scratch_elems(C.byref(a))
    assert need == (M // 8) * 32 * 2
    scratch = torch.empty(need, device="cuda")
    a.gn_scratch, a.gn_scratch_elems = scratch.data_ptr(), need - 1
    assert L.load().ldmk_post(C.byref(a), ops.stream()) == -3, "LDMK_ENOMEM: gn_scratch one float short"
    a.gn_scratch_elems = need
    ops.post(a)


# ---- LayerNorm: jn = ceil(N / 256) in 1, 1, 2, 4 (on the <5> template), 6 and 8 (on <8>) ---------------------------------------------------
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("nslab", [1, 3])
@pytest.mark.parametrize("N", [4, 256, 260, 1024, 1284, 2048])
def test_post_layernorm_template_edges(ops, request, N, nslab, data):
    from dsml_thesis_amd import lib as L
    M = 3
    base = nm.ln_input(830, M, N) if data == "mean" else rnd(830, M, N) * 1.2 + 0.3
    slabs = torch.stack([base] + [0.3 * rnd(831 + k, M, N) for k in range(1, nslab)])
    b, vec, res = 0.1 * rnd(840, N), rnd(841, 1, N), rnd(842, M, N)
    gamma, beta = 1 + 0.2 * rnd(843, N), 0.2 * rnd(844, N)
    raw_ref = slabs.double().sum(0) + b.double() + vec.double() + res.double()
    dev = [t.cuda() for t in (slabs, b, vec, res, gamma, beta)]
    outs = []
    for _ in range(2):
        raw, out = torch.full((M, N), -7.0, device="cuda"), torch.full((M, N), -7.0, device="cuda")
        ops.post(ops.make_post_args(dev[0], M, N, M, nslab=nslab, bias=dev[1], batch_vec=dev[2], batch_vec_ld=N, residual=dev[3], raw_out=raw,
                                    norm=L.POST_LAYERNORM, gamma=dev[4], beta=dev[5], eps=1e-5, norm_out=out))
        outs.append((raw, out))
    (raw, out), (raw2, out2) = outs
    assert torch.equal(raw, raw2) and torch.equal(out, out2)
    close(raw, raw_ref.float(), 1e-4, 1e-4)
    stored = raw.cpu()
    y64 = F.layer_norm(stored.double(), (N,), gamma.double(), beta.double(), 1e-5)
    mean, rstd = nm.ln_ref(stored)
    err = (out.cpu().double() - y64).abs()
    used = (err / nm.ln_out_bound(stored, mean, rstd, gamma, y64)).max().item()
    _report(request, f"norm_out ({data})", err.max().item(), used)
    assert used <= 1.0, f"norm_out uses {used:.3f} of its bound (max error {err.max().item():.3e})"
