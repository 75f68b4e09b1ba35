// First-stage (VQGAN) training: the quantiser's codebook loss with its two gradients, the backward of the narrow NCHW 1x1
// convolutions around the quantiser, and the L1 pixel loss.  gfx950 only.  No float atomics anywhere: every reduction has one
// fixed summation order, so every output is bitwise reproducible from call to call.  The sums are kept in double: these tensors
// are a few hundred KiB, the kernels are bound by launch and memory latency, and a double accumulator makes the result the
// correctly rounded one instead of one that drifts with the number of rows a code attracts.
#include "ldmk_common.h"

namespace ldmk {

// an index outside [0, n_embed) is a caller bug (ldmk_vq_nearest never writes one); clamped, it cannot become an out-of-bounds read
__device__ __forceinline__ int vq_code(int j, int n_embed) { return j < 0 ? 0 : (j >= n_embed ? n_embed - 1 : j); }

__device__ __forceinline__ double block_sum_d(double s, double* red) {      // 256 threads; the result is valid in thread 0
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------------------------------------
// VectorQuantizer2.forward (taming/modules/vqvae/quantize.py:288-296), z and dz NCHW (n, DIM, hw), idx[n*hw]:
//   dz = dzq + s (z - e_idx),  s = w c_z 2/N  (the straight-through pass plus the encoder-side term of the codebook loss)
//   partial[block] = sum (z - e_idx)^2 over the block's elements
// V = 4: 16-byte accesses, four neighbouring pixels of one channel plane (hw % 4 == 0); V = 1: the scalar form.
template <int DIM, int V>
__global__ __launch_bounds__(256) void vq_loss_bwd_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                          const int* __restrict__ idx, const float* __restrict__ dzq,
                                                          float* __restrict__ dz, int hw, int n_embed, double s,
                                                          long long total, double* __restrict__ partial) {
  __shared__ double red[4];
  const long long plane = (long long)DIM * hw;
  double sum = 0.0;
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V; i < total; i += (long long)gridDim.x * blockDim.x * V) {
    const long long b = i / plane, r = i - b * plane;
    const int d = (int)(r / hw), p = (int)(r - (long long)d * hw);
    float zv[V], gv[V], ov[V];
    int jv[V];
    if constexpr (V == 4) {
      const float4 z4 = *reinterpret_cast<const float4*>(z + i);
      const int4 j4 = *reinterpret_cast<const int4*>(idx + b * hw + p);
      zv[0] = z4.x; zv[1] = z4.y; zv[2] = z4.z; zv[3] = z4.w;
      jv[0] = j4.x; jv[1] = j4.y; jv[2] = j4.z; jv[3] = j4.w;
      if (dzq) {
        const float4 g4 = *reinterpret_cast<const float4*>(dzq + i);
        gv[0] = g4.x; gv[1] = g4.y; gv[2] = g4.z; gv[3] = g4.w;
      }
    } else {
      zv[0] = z[i];
      jv[0] = idx[b * hw + p];
      if (dzq) gv[0] = dzq[i];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const double diff = (double)zv[k] - (double)cb[(long long)vq_code(jv[k], n_embed) * DIM + d];
      sum += diff * diff;
      ov[k] = (float)((dzq ? (double)gv[k] : 0.0) + s * diff);
    }
    if (dz) {
      if constexpr (V == 4) *reinterpret_cast<float4*>(dz + i) = make_float4(ov[0], ov[1], ov[2], ov[3]);
      else dz[i] = ov[0];
    }
  }
  sum = block_sum_d(sum, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}
// loss = m + beta m with m = mean((e_idx - z)^2): both orders of the reference's two terms (legacy or not) have this value
__global__ void vq_loss_final_kernel(const double* __restrict__ partial, int blocks, double inv_n, double beta, float* __restrict__ loss) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < blocks; ++i) s += partial[i];
    const double m = s * inv_n;
    *loss = (float)(m + beta * m);
  }
}

// ---------------------------------------------------------------------------------------------
// dE[j] = s sum_{r: idx_r = j} (e_j - z_r), count[j] = |{r: idx_r = j}|.  Gather form: a workgroup owns 64 consecutive codes
// (lane <-> code) and its 16 waves split the rows.  A wave walks its rows 64 at a time: one coalesced index load, one
// compare against the tile's code range, one ballot -- with 16384 codes a 64-row step meets this tile 0.25 times on
// average, so nearly every step ends there.  A row that does hit is handed to the lane of its code (wave-uniform
// shuffles), bits in ascending order: each lane sums its rows in ascending row order, and the 16 partial sums of a code
// are added in wave order through LDS.  That order is fixed, so the result is bitwise reproducible; unused codes get exact zeros;
// a codebook that has collapsed onto one code costs rows / 16 serial adds in each wave of one workgroup, not rows.
constexpr int CG_WAVES = 16;
template <int DIM>
__global__ __launch_bounds__(64 * CG_WAVES) void vq_codebook_grad_kernel(const float* __restrict__ z, const float* __restrict__ cb,
                                                                        const int* __restrict__ idx, float* __restrict__ dE,
                                                                        int* __restrict__ count, int hw, int n_embed,
                                                                        long long rows, double s) {
  __shared__ double red[CG_WAVES][DIM][64];
  __shared__ int cnt[CG_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = blockIdx.x * 64, j = j0 + lane;
  double e[DIM], acc[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    e[d] = j < n_embed ? (double)cb[(long long)j * DIM + d] : 0.0;
    acc[d] = 0.0;
  }
  int c = 0;
  const long long steps = (rows + 63) / 64, per = (steps + CG_WAVES - 1) / CG_WAVES;
  const long long s_begin = wave * per, s_end = s_begin + per < steps ? s_begin + per : steps;
  for (long long st = s_begin; st < s_end; ++st) {
    const long long r = st * 64 + lane;
    unsigned rel = 0xFFFFFFFFu;
    float zv[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) zv[d] = 0.f;
    if (r < rows) rel = (unsigned)(vq_code(idx[r], n_embed) - j0);
    const bool hit = rel < 64u;
    if (hit) {                                   // only the rows of this tile read their latent vector
      const long long b = r / hw, p = r - b * hw;
#pragma unroll
      for (int d = 0; d < DIM; ++d) zv[d] = z[(b * DIM + d) * hw + p];
    }
    unsigned long long m = __ballot(hit);
    while (m) {
      const int src = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int t = __shfl((int)rel, src, 64);
      float zs[DIM];
#pragma unroll
      for (int d = 0; d < DIM; ++d) zs[d] = __shfl(zv[d], src, 64);
      if (lane == t) {
#pragma unroll
        for (int d = 0; d < DIM; ++d) acc[d] += e[d] - (double)zs[d];
        ++c;
      }
    }
  }
#pragma unroll
  for (int d = 0; d < DIM; ++d) red[wave][d][lane] = acc[d];
  cnt[wave][lane] = c;
  __syncthreads();
  if (wave == 0 && j < n_embed) {
    int ct = 0;
    for (int w = 0; w < CG_WAVES; ++w) ct += cnt[w][lane];
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      double t = 0.0;
      for (int w = 0; w < CG_WAVES; ++w) t += red[w][d][lane];
      dE[(long long)j * DIM + d] = ct ? (float)(t * s) : 0.f;
    }
    if (count) count[j] = ct;
  }
}

// ---------------------------------------------------------------------------------------------
// Backward of ldmk_conv1x1_nchw (quant_conv / post_quant_conv, autoencoder.py:61-62), cin, cout <= 8, thread <-> pixel:
//   dx[b][c][p] = sum_co w[co][c] dy[b][co][p]     (fp32 fused multiply-add chain, co ascending)
//   dW[co][c]   = sum_{b,p} dy[b][co][p] x[b][c][p],  db[co] = sum_{b,p} dy[b][co][p]
// The 72 sums are kept per thread in double, reduced over the workgroup in a fixed order and written as one row of
// `partial` per workgroup; conv1x1_bwd_final_kernel adds the rows in workgroup order.
constexpr int C11_MAX = 8, C11_ROW = C11_MAX * C11_MAX + C11_MAX, C11_BLOCKS = 128;
__global__ __launch_bounds__(256) void conv1x1_nchw_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                               const float* __restrict__ w, float* __restrict__ dx, int hw,
                                                               int cin, int cout, long long pixels, int params,
                                                               double* __restrict__ partial) {
  __shared__ double red[4];
  double aw[C11_MAX][C11_MAX], ab[C11_MAX];
#pragma unroll
  for (int co = 0; co < C11_MAX; ++co) {
    ab[co] = 0.0;
#pragma unroll
    for (int c = 0; c < C11_MAX; ++c) aw[co][c] = 0.0;
  }
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / hw, p = i - b * hw;
    float xv[C11_MAX], gv[C11_MAX];
#pragma unroll
    for (int c = 0; c < C11_MAX; ++c) xv[c] = (x && c < cin) ? x[(b * cin + c) * hw + p] : 0.f;   // x null: db alone
#pragma unroll
    for (int co = 0; co < C11_MAX; ++co) gv[co] = co < cout ? dy[(b * cout + co) * hw + p] : 0.f;
    if (dx) {
#pragma unroll
      for (int c = 0; c < C11_MAX; ++c) {
        if (c < cin) {
          float a = 0.f;
#pragma unroll
          for (int co = 0; co < C11_MAX; ++co)
            if (co < cout) a = fmaf(w[co * cin + c], gv[co], a);
          dx[(b * cin + c) * hw + p] = a;
        }
      }
    }
    if (params) {
#pragma unroll
      for (int co = 0; co < C11_MAX; ++co) {
        ab[co] += (double)gv[co];
#pragma unroll
        for (int c = 0; c < C11_MAX; ++c) aw[co][c] += (double)gv[co] * (double)xv[c];
      }
    }
  }
  if (!params) return;
  double* row = partial + (long long)blockIdx.x * C11_ROW;
#pragma unroll
  for (int co = 0; co < C11_MAX; ++co) {
    if (co >= cout) break;                              // (uniform)
#pragma unroll
    for (int c = 0; c < C11_MAX; ++c) {
      if (c >= cin) break;
      __syncthreads();                                  // red is free again
      const double t = block_sum_d(aw[co][c], red);
      if (threadIdx.x == 0) row[co * C11_MAX + c] = t;
    }
    __syncthreads();
    const double t = block_sum_d(ab[co], red);
    if (threadIdx.x == 0) row[C11_MAX * C11_MAX + co] = t;
  }
}
__global__ void conv1x1_bwd_final_kernel(const double* __restrict__ partial, int blocks, int cin, int cout, float* __restrict__ dw,
                                         float* __restrict__ db, int accumulate) {
  const int t = threadIdx.x;
  if (t >= C11_ROW) return;
  const bool bias = t >= C11_MAX * C11_MAX;
  const int co = bias ? t - C11_MAX * C11_MAX : t / C11_MAX, c = bias ? 0 : t % C11_MAX;
  if (co >= cout || c >= cin) return;
  float* dst = bias ? (db ? db + co : nullptr) : (dw ? dw + co * cin + c : nullptr);
  if (!dst) return;
  double s = 0.0;
  for (int i = 0; i < blocks; ++i) s += partial[(long long)i * C11_ROW + t];
  *dst = accumulate ? *dst + (float)s : (float)s;
}

// ---------------------------------------------------------------------------------------------
// mean-absolute-error loss (the 'l1' pixel loss, vqperceptual.py:28-31,82): dpred = sign(pred - target) / denom with
// sign(0) = 0 as torch.sign has it (a NaN difference stays a NaN), loss partials per workgroup
__global__ __launch_bounds__(256) void l1_grad_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                      float* __restrict__ dpred, long long n, float g,
                                                      double* __restrict__ partial) {
  __shared__ double red[4];
  double s = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float d = pred[i] - target[i];
    dpred[i] = d > 0.f ? g : (d < 0.f ? -g : d * 0.f);
    s += (double)fabsf(d);
  }
  s = block_sum_d(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ void l1_final_kernel(const double* __restrict__ partial, int blocks, double inv_n, float* __restrict__ loss) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < blocks; ++i) s += partial[i];
    *loss = (float)(s * inv_n);
  }
}

}  // namespace ldmk

using namespace ldmk;

extern "C" int ldmk_vq_loss_bwd(const float* z, const float* codebook, const int* idx, const float* dzq, float* dz, float* loss,
                                int n, int hw, int dim, int n_embed, float beta, int legacy, float w, double* scratch,
                                void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(dim == 3 || dim == 4, "ldmk_vq_loss_bwd: embed dim %d unsupported (3 or 4)", dim);
  LDMK_REQUIRE(z && codebook && idx && loss && scratch && n > 0 && hw > 0 && n_embed > 0, "ldmk_vq_loss_bwd: bad args");
  LDMK_REQUIRE(dz || !dzq, "ldmk_vq_loss_bwd: dzq without dz");
  const long long total = (long long)n * dim * hw;
  const double s = (double)w * (legacy ? 1.0 : (double)beta) * 2.0 / (double)total;
  auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  const bool vec = hw % 4 == 0 && al(z) && al(idx) && al(dzq) && al(dz);
  long long g = ((vec ? total / 4 : total) + 255) / 256;
  const int blocks = (int)(g > 256 ? 256 : g);                 // scratch: 256 doubles
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(blocks), block(256);
  if (dim == 3) {
    if (vec) hipLaunchKernelGGL((vq_loss_bwd_kernel<3, 4>), grid, block, 0, st, z, codebook, idx, dzq, dz, hw, n_embed, s, total, scratch);
    else hipLaunchKernelGGL((vq_loss_bwd_kernel<3, 1>), grid, block, 0, st, z, codebook, idx, dzq, dz, hw, n_embed, s, total, scratch);
  } else {
    if (vec) hipLaunchKernelGGL((vq_loss_bwd_kernel<4, 4>), grid, block, 0, st, z, codebook, idx, dzq, dz, hw, n_embed, s, total, scratch);
    else hipLaunchKernelGGL((vq_loss_bwd_kernel<4, 1>), grid, block, 0, st, z, codebook, idx, dzq, dz, hw, n_embed, s, total, scratch);
  }
  hipLaunchKernelGGL(vq_loss_final_kernel, dim3(1), dim3(64), 0, st, scratch, blocks, 1.0 / (double)total, (double)beta, loss);
  return check_launch("ldmk_vq_loss_bwd");
}

extern "C" int ldmk_vq_codebook_grad(const float* z, const float* codebook, const int* idx, float* dE, int* count, int n, int hw,
                                     int dim, int n_embed, float beta, int legacy, float w, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(dim == 3 || dim == 4, "ldmk_vq_codebook_grad: embed dim %d unsupported (3 or 4)", dim);
  LDMK_REQUIRE(z && codebook && idx && dE && n > 0 && hw > 0 && n_embed > 0, "ldmk_vq_codebook_grad: bad args");
  const long long rows = (long long)n * hw;
  const double s = (double)w * (legacy ? (double)beta : 1.0) * 2.0 / ((double)rows * dim);
  const dim3 grid((unsigned)((n_embed + 63) / 64)), block(64 * CG_WAVES);
  hipStream_t st = (hipStream_t)stream;
  if (dim == 3) hipLaunchKernelGGL(vq_codebook_grad_kernel<3>, grid, block, 0, st, z, codebook, idx, dE, count, hw, n_embed, rows, s);
  else hipLaunchKernelGGL(vq_codebook_grad_kernel<4>, grid, block, 0, st, z, codebook, idx, dE, count, hw, n_embed, rows, s);
  return check_launch("ldmk_vq_codebook_grad");
}

extern "C" int ldmk_conv1x1_nchw_bwd(const float* x, const float* dy, const float* w, float* dx, float* dw, float* db, int n,
                                     int hw, int cin, int cout, int accumulate, double* scratch, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(cin >= 1 && cin <= C11_MAX && cout >= 1 && cout <= C11_MAX,
               "ldmk_conv1x1_nchw_bwd: cin=%d, cout=%d must be in [1, %d]", cin, cout, C11_MAX);
  LDMK_REQUIRE(dy && n > 0 && hw > 0, "ldmk_conv1x1_nchw_bwd: bad args");
  LDMK_REQUIRE(dx || dw || db, "ldmk_conv1x1_nchw_bwd: no output requested");
  LDMK_REQUIRE(!dx || w, "ldmk_conv1x1_nchw_bwd: dx needs the weight");
  LDMK_REQUIRE(!dw || x, "ldmk_conv1x1_nchw_bwd: dw needs the forward input");
  const int params = (dw || db) ? 1 : 0;
  LDMK_REQUIRE(!params || scratch, "ldmk_conv1x1_nchw_bwd: dw / db need the scratch");
  const long long pixels = (long long)n * hw;
  const long long g = (pixels + 255) / 256;
  const int blocks = (int)(g > C11_BLOCKS ? C11_BLOCKS : g);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(conv1x1_nchw_bwd_kernel, dim3(blocks), dim3(256), 0, st, dw ? x : nullptr, dy, w, dx, hw, cin, cout, pixels,
                     params, scratch);
  if (params)
    hipLaunchKernelGGL(conv1x1_bwd_final_kernel, dim3(1), dim3(128), 0, st, scratch, blocks, cin, cout, dw, db, accumulate);
  return check_launch("ldmk_conv1x1_nchw_bwd");
}

extern "C" int ldmk_l1_grad(const float* pred, const float* target, float* dpred, long long n, long long denom, float* loss,
                            double* scratch, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(pred && target && dpred && loss && scratch && n > 0 && denom >= 0, "ldmk_l1_grad: bad args");
  if (denom == 0) denom = n;                                 // channel-padded tensors: mean over the real elements only
  const int blocks = 256;                                    // scratch: 256 doubles
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(l1_grad_kernel, dim3(blocks), dim3(256), 0, st, pred, target, dpred, n, (float)(1.0 / (double)denom), scratch);
  hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(64), 0, st, scratch, blocks, 1.0 / (double)denom, loss);
  return check_launch("ldmk_l1_grad");
}
