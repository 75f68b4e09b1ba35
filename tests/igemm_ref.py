"""Plain float64 reference of ldmk_igemm (include/ldmk.h) for tests/test_igemm_edges_gpu.py; checked on the CPU by
tests/test_igemm_ref_cpu.py.

    out[M][N] = alpha * transform(A)[M][K] @ W[K][N] + bias + batch_vec[row // rows_per_sample] + residual

transform(A) is built EXPLICITLY, element by element from index arithmetic written down here (no F.conv2d, F.pad or
F.interpolate): the channel concat of the two sources, the optional per-sample affine (scale, shift), then -- conv mode -- the
nine taps of every output pixel in the K order ops.pack_conv3x3 documents, [C / 32][9][32]: k = (c // 32 * 9 + 3 dy + dx) * 32 +
c % 32.  A tap outside the (virtual) image is zero AFTER the affine (the convolution pads the transformed tensor)."""
import torch


def concat_affine(x0, x1=None, coef=None):
    """x0 [n, ..., c0] (+ x1 [n, ..., c1]) -> float64 [n, ..., c0 + c1]; coef [n][2][C] (scale plane, shift plane) applied per sample."""
    x = x0.double() if x1 is None else torch.cat([x0.double(), x1.double()], -1)
    if coef is not None:
        shape = (x.shape[0],) + (1,) * (x.dim() - 2) + (x.shape[-1],)
        x = x * coef[:, 0].double().reshape(shape) + coef[:, 1].double().reshape(shape)
    return x


def out_size(size, stride, pad_lo, upsample):
    """Output extent of the 3x3 window along one axis: nn.Conv2d(padding=1) for pad_lo = 1, F.pad(0, 1) + padding 0 for pad_lo = 0,
    on the (virtually x2 enlarged, upsample != 0) input."""
    v = 2 * size if upsample else size
    return (v + 2 - 3) // stride + 1 if pad_lo == 1 else (v + 1 - 3) // stride + 1


def conv_operand(x, stride=1, pad_lo=1, upsample=0):
    """x: float64 [n][h][w][C] (C % 32 == 0), already concatenated and transformed -> (A [n oh ow][9 C], oh, ow).
    iy = oy * stride + dy - pad_lo in the virtual grid (2h x 2w when upsample != 0); upsample 1 reads pixel (iy // 2, ix // 2),
    upsample 2 reads it only where iy and ix are both even (zero insertion)."""
    n, h, w, C = x.shape
    assert C % 32 == 0
    vh, vw = (2 * h, 2 * w) if upsample else (h, w)
    oh, ow = out_size(h, stride, pad_lo, upsample), out_size(w, stride, pad_lo, upsample)
    A = torch.zeros(n, oh, ow, C // 32, 9, 32, dtype=torch.float64)
    xc = x.reshape(n, h, w, C // 32, 32)
    for oy in range(oh):
        for ox in range(ow):
            for dy in range(3):
                for dx in range(3):
                    iy, ix = oy * stride + dy - pad_lo, ox * stride + dx - pad_lo
                    if iy < 0 or ix < 0 or iy >= vh or ix >= vw:
                        continue
                    if upsample == 2 and (iy % 2 or ix % 2):
                        continue
                    sy, sx = (iy // 2, ix // 2) if upsample else (iy, ix)
                    A[:, oy, ox, :, 3 * dy + dx, :] = xc[:, sy, sx]
    return A.reshape(n * oh * ow, 9 * C), oh, ow


def operand_matrix(x0, x1=None, coef=None, conv=None, rows_per_sample=None, skip=None):
    """transform(A)[M][K] in float64.
    rows mode (conv None): x0 [M][c0] (+ x1 [M][c1]); coef [n][2][K] applies to row r with sample r // rows_per_sample.
    conv mode: x0 [n][h][w][c0] (+ x1), conv = (stride, pad_lo, upsample).
    skip: [M][skip_c] rows appended as trailing K columns (the fused 1x1 skip connection of the slab tiles)."""
    if conv is None:
        A = concat_affine(x0, x1)
        if coef is not None:
            smp = torch.arange(A.shape[0]) // rows_per_sample
            A = A * coef[smp, 0].double() + coef[smp, 1].double()
    else:
        A = conv_operand(concat_affine(x0, x1, coef), *conv)[0]
    if skip is not None:
        A = torch.cat([A, skip.double()], 1)
    return A


def igemm_ref(A, W, alpha=1.0, bias=None, batch_vec=None, rows_per_sample=None, residual=None):
    """alpha * A @ W + bias + batch_vec[row // rows_per_sample] + residual, float64.  W: [K][N]."""
    out = alpha * (A.double() @ W.double())
    if bias is not None:
        out = out + bias.double()
    if batch_vec is not None:
        out = out + batch_vec.double()[torch.arange(A.shape[0]) // rows_per_sample]
    if residual is not None:
        out = out + residual.double()
    return out


def geglu_ref(y, inner):
    """GEGLU epilogue on y [M][2 inner] whose columns are packed by ops.pack_geglu (32 value columns | their 32 gates):
    out[:, 32 b + j] = y[:, 64 b + j] * gelu(y[:, 64 b + 32 + j]) (exact erf GELU)."""
    t = y.reshape(y.shape[0], inner // 32, 2, 32)
    return (t[:, :, 0] * torch.nn.functional.gelu(t[:, :, 1])).reshape(y.shape[0], inner)


# ---- the PS layout (include/ldmk.h): plane g of element (r, k) of X[R][K] is the 16-bit word at
#     (((r / 32) (K / 16) + k / 16) planes + g) 512 + ((k / 8 % 2) 32 + r % 32) 8 + k % 8
def ps_index(r, k, K, g, planes=3):
    return (((r // 32) * (K // 16) + k // 16) * planes + g) * 512 + ((k // 8 % 2) * 32 + r % 32) * 8 + k % 8


def ps_words(rows, K, planes=3):
    """Number of 16-bit words of the PS layout of a [rows][K] matrix (ldmk_ps_bytes / 2)."""
    return ((rows + 31) // 32) * (K // 16) * planes * 512


def ps_row_words(r, K, planes=3):
    """Indices of every 16-bit word that belongs to row r (all k, all planes)."""
    k = torch.arange(K)
    return torch.cat([ps_index(r, k, K, g, planes) for g in range(planes)])


def split3(x):
    """The exact three-way bf16 split: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), round to nearest even."""
    hi = x.to(torch.bfloat16)
    r = x - hi.float()
    mid = r.to(torch.bfloat16)
    lo = (r - mid.float()).to(torch.bfloat16)
    return hi, mid, lo


def pack_ps_ref(x):
    """fp32 [rows][K] -> the bf16 PS tensor (1-d, ps_words elements), written word by word with ps_index; padding rows zero."""
    rows, K = x.shape
    out = torch.zeros(ps_words(rows, K), dtype=torch.bfloat16)
    r, k = torch.meshgrid(torch.arange(rows), torch.arange(K), indexing="ij")
    for g, plane in enumerate(split3(x.float())):
        out[ps_index(r, k, K, g).reshape(-1)] = plane.reshape(-1)
    return out
