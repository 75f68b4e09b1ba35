"""CPU: the float64 reference of tests/igemm_ref.py is held to three independent statements, each bitwise on integer data, so that
tests/test_igemm_edges_gpu.py can trust it: (1) F.conv2d in float64 (with F.pad, F.interpolate and zero insertion as the case
needs) over every geometry the GPU module uses; (2) the K order of _pack_ref (what ops.pack_conv3x3 documents); (3) the PS index
formula of include/ldmk.h against the reshape-based ops.unpack_ps."""
import pytest
import torch
import torch.nn.functional as F

import igemm_ref as R
from test_backward_edges_gpu import _ints, _pack_ref

# (n, h, w, stride, pad_lo, upsample): the images and geometries of test_igemm_edges_gpu.py
GEOMETRIES = ([(n, h, w, 1, 1, 0) for n in (1, 3) for h, w in ((1, 1), (1, 5), (5, 1), (3, 8), (5, 7))] +
              [(2, h, w, 2, p, 0) for h, w in ((5, 7), (6, 4)) for p in (1, 0)] +
              [(2, 3, 5, 1, 1, 1), (1, 1, 1, 1, 1, 1), (2, 3, 5, 1, 1, 2), (1, 2, 2, 2, 0, 1)])


def _torch_conv(x, wt, stride, pad_lo, upsample):
    """x float64 NCHW (already transformed), wt OIHW -> NHWC rows [n oh ow][O] through torch's own convolution."""
    if upsample == 1:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    elif upsample == 2:
        z = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3], dtype=x.dtype)
        z[:, :, ::2, ::2] = x
        x = z
    y = F.conv2d(x, wt, None, stride=stride, padding=1) if pad_lo == 1 else F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, None, stride=stride)
    return y.permute(0, 2, 3, 1).reshape(-1, wt.shape[0]), y.shape[2], y.shape[3]


@pytest.mark.parametrize("two_sources,affine", [(False, False), (True, True)])
@pytest.mark.parametrize("geo", GEOMETRIES)
def test_conv_operand_matches_conv2d(geo, two_sources, affine):
    n, h, w, stride, pad_lo, ups = geo
    c0, c1, O = 32, (64 if two_sources else 0), 8
    C = c0 + c1
    x0 = _ints(900, n, h, w, c0)
    x1 = _ints(901, n, h, w, c1) if c1 else None
    coef = None
    if affine:                                                # scale in {1, 2, -1}, integer shift: the shifted border must still read 0
        coef = torch.stack([torch.tensor([1.0, 2.0, -1.0])[_ints(902, n, C, lo=0, hi=2).long()], _ints(903, n, C, lo=-3, hi=3)], 1)
    wt = _ints(904, O, C, 3, 3).double()
    A = R.operand_matrix(x0, x1, coef=coef, conv=(stride, pad_lo, ups))
    xt = R.concat_affine(x0, x1, coef).permute(0, 3, 1, 2)
    ref, oh, ow = _torch_conv(xt, wt, stride, pad_lo, ups)
    assert (oh, ow) == (R.out_size(h, stride, pad_lo, ups), R.out_size(w, stride, pad_lo, ups))
    assert A.shape == (n * oh * ow, 9 * C)
    got = R.igemm_ref(A, _pack_ref(wt))
    assert torch.equal(got, ref), "operand matrix x packed weights != F.conv2d"
    if affine and pad_lo == 1 and not ups:
        assert (A[0].reshape(C // 32, 9, 32)[:, 0] == 0).all(), "the halo is zero after the affine, not shift"


def test_k_order_is_the_one_of_pack_ref():
    """A one-hot weight at (o, c, dy, dx) lands in row (c // 32 * 9 + 3 dy + dx) * 32 + c % 32 of _pack_ref -- the k the builder uses."""
    O, C = 4, 96
    for (o, c, dy, dx) in [(0, 0, 0, 0), (1, 33, 1, 2), (3, 95, 2, 0), (2, 64, 2, 2)]:
        wt = torch.zeros(O, C, 3, 3)
        wt[o, c, dy, dx] = 1.0
        k = (c // 32 * 9 + 3 * dy + dx) * 32 + c % 32
        hot = _pack_ref(wt).nonzero().tolist()
        assert hot == [[k, o]]
        x = _ints(905, 1, 3, 3, C)
        A = R.operand_matrix(x, conv=(1, 1, 0))
        assert torch.equal(A[4, k], x[0, dy, dx, c].double())      # centre pixel (1, 1): tap (dy, dx) reads pixel (dy, dx)


def test_rows_mode_epilogue_terms():
    M, c0, c1, N, rps = 11, 32, 64, 8, 5
    x0, x1 = _ints(910, M, c0), _ints(911, M, c1)
    n = -(-M // rps)
    coef = torch.stack([2.0 * torch.ones(n, c0 + c1), _ints(912, n, c0 + c1)], 1)
    W, b, v, r = _ints(913, c0 + c1, N), _ints(914, N), _ints(915, n, N), _ints(916, M, N)
    A = R.operand_matrix(x0, x1, coef=coef, rows_per_sample=rps)
    got = R.igemm_ref(A, W, alpha=0.5, bias=b, batch_vec=v, rows_per_sample=rps, residual=r)
    for m in (0, 4, 5, 10):
        s = m // rps
        a = torch.cat([x0[m], x1[m]]).double() * 2.0 + coef[s, 1].double()
        assert torch.equal(got[m], 0.5 * (a @ W.double()) + b.double() + v[s].double() + r[m].double())
    skip = _ints(917, M, 16)
    assert torch.equal(R.operand_matrix(x0, skip=skip)[:, c0:], skip.double())


@pytest.mark.parametrize("rows,K", [(33, 32), (64, 96), (1, 16)])
def test_ps_index_formula(rows, K):
    """pack_ps_ref writes word by word with the formula of ldmk.h; ops.unpack_ps reads with a reshape: they must agree, the
    row words of ps_row_words are exactly the words of that row, and rows >= `rows` are the padding of the last 32-row block."""
    from dsml_thesis_amd import ops
    x = _ints(920, rows, K) * 1.001
    ps = R.pack_ps_ref(x)
    assert ps.numel() == R.ps_words(rows, K) == ((rows + 31) // 32) * (K // 16) * 1536
    hi, mid, lo = ops.unpack_ps(ps.view(torch.uint8), rows, K)
    assert torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    rh, rm, rl = R.split3(x)
    assert torch.equal(hi, rh.float()) and torch.equal(mid, rm.float()) and torch.equal(lo, rl.float())
    seen = torch.cat([R.ps_row_words(r, K) for r in range(32 * ((rows + 31) // 32))])
    assert seen.numel() == ps.numel() and torch.equal(seen.sort().values, torch.arange(ps.numel())), "the formula is a bijection"
    marked = ps.clone()
    marked[R.ps_row_words(rows - 1, K)] = 7.0
    h2, m2, l2 = ops.unpack_ps(marked.view(torch.uint8), rows, K)
    assert (h2[rows - 1] == 7).all() and torch.equal(h2[:rows - 1], hi[:rows - 1])


@pytest.mark.parametrize("rows,K", [(33, 32), (64, 96), (1, 16)])
def test_ps_index_formula_two_planes(rows, K):
    """The F16X2 form of the layout (two fp16 planes per unit): words written one by one with ps_index(planes=2) read back through
    ops.unpack_ps_h2; ps_row_words(planes=2) are exactly a row's words -- what the conv-mode padding test poisons through."""
    from dsml_thesis_amd import ops
    nb = (rows + 31) // 32
    assert R.ps_words(rows, K, 2) == nb * (K // 16) * 1024
    hi, lo = _ints(921, rows, K, lo=-9, hi=9).half(), (_ints(922, rows, K, lo=-9, hi=9) / 64).half()
    ps = torch.zeros(R.ps_words(rows, K, 2), dtype=torch.float16)
    r, k = torch.meshgrid(torch.arange(rows), torch.arange(K), indexing="ij")
    for g, plane in enumerate((hi, lo)):
        ps[R.ps_index(r, k, K, g, 2).reshape(-1)] = plane.reshape(-1)
    gh, gl = ops.unpack_ps_h2(ps.view(torch.uint8), rows, K)
    assert torch.equal(gh, hi.float()) and torch.equal(gl, lo.float())
    seen = torch.cat([R.ps_row_words(r_, K, 2) for r_ in range(32 * nb)])
    assert seen.numel() == ps.numel() and torch.equal(seen.sort().values, torch.arange(ps.numel())), "the formula is a bijection"
    marked = ps.clone()
    marked[R.ps_row_words(rows - 1, K, 2)] = 7.0
    h2, l2 = ops.unpack_ps_h2(marked.view(torch.uint8), rows, K)
    assert (h2[rows - 1] == 7).all() and (l2[rows - 1] == 7).all() and torch.equal(h2[:rows - 1], gh[:rows - 1])
    if rows % 32:                                             # a padding row's words touch no real row
        marked = ps.clone()
        marked[R.ps_row_words(rows, K, 2)] = 7.0
        h3, l3 = ops.unpack_ps_h2(marked.view(torch.uint8), rows, K)
        assert torch.equal(h3, gh) and torch.equal(l3, gl)


def test_geglu_ref_pairs():
    y = _ints(930, 3, 128).double()
    out = R.geglu_ref(y, 64)
    assert torch.equal(out[:, 40], y[:, 72] * F.gelu(y[:, 104]))
