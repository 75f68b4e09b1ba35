// First-stage (KL) training: the diagonal-Gaussian bottleneck of AutoencoderKL with its KL term (distributions.py:24-49) forward
// and backward, and the L1 pixel term of the NLL loss with a real-valued gradient scale (contperceptual.py:48-58).  gfx950 only.
// The conventions of vq_train.hip: fp32 in and out, no float atomics, every sum kept in double in one fixed order (per-workgroup
// partials in a caller-supplied scratch, added in workgroup order by a final kernel), so every output is bitwise reproducible.
// V = 4: 16-byte accesses; V = 1: the scalar form for planes that are no multiple of 4 floats or pointers off a 16-byte boundary.
#include "ldmk_common.h"

namespace ldmk {

constexpr int KL_BPS = 64;          // workgroups per sample at the most (scratch: n * KL_BPS doubles)
constexpr int L1S_BLOCKS = 256;     // workgroups of the pixel term at the most (scratch: 256 doubles)

__device__ __forceinline__ double kl_block_sum_d(double s, double* red) {   // 256 threads; the result is valid in thread 0
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------------------------------------
// moments (n, 2e, hw) = [mean | raw log-variance], plane = e*hw.  Workgroup (x, b) walks sample b's plane with stride gridDim.x:
//   lv = clamp(raw, -30, 20), std = expf(0.5 lv), z = fmaf(std, noise, mean) (noise null: mean) -- gauss_posterior_kernel's
//   arithmetic at scale 1, bit for bit;
//   partial[b][x] = sum over the workgroup's elements of mean^2 + exp(lv) - 1 - lv, each term and the sum in double.
template <int V>
__global__ __launch_bounds__(256) void gauss_kl_fwd_kernel(const float* __restrict__ moments, const float* __restrict__ noise,
                                                           float* __restrict__ z, long long plane, double* __restrict__ partial) {
  __shared__ double red[4];
  const long long b = blockIdx.y;
  const float* mp = moments + b * 2 * plane;
  double sum = 0.0;
  for (long long r = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V; r < plane; r += (long long)gridDim.x * blockDim.x * V) {
    float mean[V], lv[V], nz[V], zz[V];
    if constexpr (V == 4) {
      const float4 m4 = *reinterpret_cast<const float4*>(mp + r), l4 = *reinterpret_cast<const float4*>(mp + plane + r);
      mean[0] = m4.x; mean[1] = m4.y; mean[2] = m4.z; mean[3] = m4.w;
      lv[0] = l4.x; lv[1] = l4.y; lv[2] = l4.z; lv[3] = l4.w;
      if (noise) {
        const float4 n4 = *reinterpret_cast<const float4*>(noise + b * plane + r);
        nz[0] = n4.x; nz[1] = n4.y; nz[2] = n4.z; nz[3] = n4.w;
      }
    } else {
      mean[0] = mp[r];
      lv[0] = mp[plane + r];
      if (noise) nz[0] = noise[b * plane + r];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      lv[k] = fminf(fmaxf(lv[k], -30.0f), 20.0f);
      zz[k] = noise ? fmaf(expf(0.5f * lv[k]), nz[k], mean[k]) : mean[k];
      const double m = (double)mean[k], l = (double)lv[k];
      sum += m * m + exp(l) - 1.0 - l;
    }
    if constexpr (V == 4) *reinterpret_cast<float4*>(z + b * plane + r) = make_float4(zz[0], zz[1], zz[2], zz[3]);
    else z[b * plane + r] = zz[0];
  }
  sum = kl_block_sum_d(sum, red);
  if (threadIdx.x == 0) partial[b * gridDim.x + blockIdx.x] = sum;
}
__global__ void gauss_kl_final_kernel(const double* __restrict__ partial, int n, int bps, float* __restrict__ kl) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  double s = 0.0;
  for (int i = 0; i < bps; ++i) s += partial[(long long)b * bps + i];
  kl[b] = (float)(0.5 * s);
}

// dmoments (n, 2e, hw):  d mean = dz + w mean;  d raw log-variance = 0.5 (dz noise std + w (var - 1)) where the raw value lies in
// [-30, 20] (bounds included: torch.clamp passes the gradient there) and 0 elsewhere.  dz null: the KL term alone; noise null
// (the posterior's mode was decoded): no std term.  fp32, one fused multiply-add per sum.
template <int V>
__global__ __launch_bounds__(256) void gauss_kl_bwd_kernel(const float* __restrict__ moments, const float* __restrict__ noise,
                                                           const float* __restrict__ dz, float w, float* __restrict__ dmoments,
                                                           long long plane, long long total) {
  const bool sampled = noise && dz;
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V; i < total; i += (long long)gridDim.x * blockDim.x * V) {
    const long long b = i / plane, r = i - b * plane;
    const float* mp = moments + b * 2 * plane + r;
    float* op = dmoments + b * 2 * plane + r;
    float mean[V], raw[V], nz[V], g[V], dm[V], dl[V];
    if constexpr (V == 4) {
      const float4 m4 = *reinterpret_cast<const float4*>(mp), l4 = *reinterpret_cast<const float4*>(mp + plane);
      mean[0] = m4.x; mean[1] = m4.y; mean[2] = m4.z; mean[3] = m4.w;
      raw[0] = l4.x; raw[1] = l4.y; raw[2] = l4.z; raw[3] = l4.w;
      if (dz) {
        const float4 g4 = *reinterpret_cast<const float4*>(dz + i);
        g[0] = g4.x; g[1] = g4.y; g[2] = g4.z; g[3] = g4.w;
      }
      if (sampled) {
        const float4 n4 = *reinterpret_cast<const float4*>(noise + i);
        nz[0] = n4.x; nz[1] = n4.y; nz[2] = n4.z; nz[3] = n4.w;
      }
    } else {
      mean[0] = mp[0];
      raw[0] = mp[plane];
      if (dz) g[0] = dz[i];
      if (sampled) nz[0] = noise[i];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float gk = dz ? g[k] : 0.f;
      dm[k] = fmaf(w, mean[k], gk);
      const bool inside = raw[k] >= -30.0f && raw[k] <= 20.0f;
      const float klt = w * (expf(raw[k]) - 1.0f);                 // (inside: the raw value is the clamped one)
      const float t = sampled ? fmaf(gk * nz[k], expf(0.5f * raw[k]), klt) : klt;
      dl[k] = inside ? 0.5f * t : 0.f;
    }
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(op) = make_float4(dm[0], dm[1], dm[2], dm[3]);
      *reinterpret_cast<float4*>(op + plane) = make_float4(dl[0], dl[1], dl[2], dl[3]);
    } else {
      op[0] = dm[0];
      op[plane] = dl[0];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The pixel term of the NLL (contperceptual.py:48,53-58): dpred = g sign(pred - target) with sign(0) = 0 as torch.sign has it
// (a NaN difference stays a NaN), partial[block] = sum |pred - target|.  l1_grad_kernel (vq_train.hip) with a caller's scale.
template <int V>
__global__ __launch_bounds__(256) void l1_sum_grad_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                          float* __restrict__ dpred, long long n, float g,
                                                          double* __restrict__ partial) {
  __shared__ double red[4];
  double s = 0.0;
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V; i < n; i += (long long)gridDim.x * blockDim.x * V) {
    float p[V], t[V], o[V];
    if constexpr (V == 4) {
      const float4 p4 = *reinterpret_cast<const float4*>(pred + i), t4 = *reinterpret_cast<const float4*>(target + i);
      p[0] = p4.x; p[1] = p4.y; p[2] = p4.z; p[3] = p4.w;
      t[0] = t4.x; t[1] = t4.y; t[2] = t4.z; t[3] = t4.w;
    } else {
      p[0] = pred[i];
      t[0] = target[i];
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float d = p[k] - t[k];
      o[k] = d > 0.f ? g : (d < 0.f ? -g : d * 0.f);
      s += (double)fabsf(d);
    }
    if constexpr (V == 4) *reinterpret_cast<float4*>(dpred + i) = make_float4(o[0], o[1], o[2], o[3]);
    else dpred[i] = o[0];
  }
  s = kl_block_sum_d(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ void l1_sum_final_kernel(const double* __restrict__ partial, int blocks, float* __restrict__ sum) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < blocks; ++i) s += partial[i];
    *sum = (float)s;
  }
}

}  // namespace ldmk

using namespace ldmk;

static inline bool kl_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int ldmk_gauss_kl_fwd(const float* moments, const float* noise, float* z, float* kl, int n, int e, int hw,
                                 double* scratch, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(moments && z && kl && scratch && n > 0 && e > 0 && hw > 0, "ldmk_gauss_kl_fwd: bad args");
  LDMK_REQUIRE(n <= 65535, "ldmk_gauss_kl_fwd: n=%d above 65535 samples", n);
  const long long plane = (long long)e * hw;
  const bool vec = plane % 4 == 0 && kl_al16(moments) && kl_al16(noise) && kl_al16(z);
  long long g = ((vec ? plane / 4 : plane) + 255) / 256;
  const int bps = (int)(g > KL_BPS ? KL_BPS : g);
  const dim3 grid((unsigned)bps, (unsigned)n), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(gauss_kl_fwd_kernel<4>, grid, block, 0, st, moments, noise, z, plane, scratch);
  else hipLaunchKernelGGL(gauss_kl_fwd_kernel<1>, grid, block, 0, st, moments, noise, z, plane, scratch);
  hipLaunchKernelGGL(gauss_kl_final_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, scratch, n, bps, kl);
  return check_launch("ldmk_gauss_kl_fwd");
}

extern "C" int ldmk_gauss_kl_bwd(const float* moments, const float* noise, const float* dz, float w, float* dmoments, int n,
                                 int e, int hw, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(moments && dmoments && n > 0 && e > 0 && hw > 0, "ldmk_gauss_kl_bwd: bad args");
  const long long plane = (long long)e * hw, total = plane * n;
  const bool vec = plane % 4 == 0 && kl_al16(moments) && kl_al16(noise) && kl_al16(dz) && kl_al16(dmoments);
  long long g = ((vec ? total / 4 : total) + 255) / 256;
  if (g > 4096) g = 4096;
  const dim3 grid((unsigned)g), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(gauss_kl_bwd_kernel<4>, grid, block, 0, st, moments, noise, dz, w, dmoments, plane, total);
  else hipLaunchKernelGGL(gauss_kl_bwd_kernel<1>, grid, block, 0, st, moments, noise, dz, w, dmoments, plane, total);
  return check_launch("ldmk_gauss_kl_bwd");
}

extern "C" int ldmk_l1_sum_grad(const float* pred, const float* target, float* dpred, long long n, float g, float* sum,
                                double* scratch, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(pred && target && dpred && sum && scratch && n > 0, "ldmk_l1_sum_grad: bad args");
  const bool vec = n % 4 == 0 && kl_al16(pred) && kl_al16(target) && kl_al16(dpred);
  long long b = ((vec ? n / 4 : n) + 255) / 256;
  const int blocks = (int)(b > L1S_BLOCKS ? L1S_BLOCKS : b);
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(l1_sum_grad_kernel<4>, dim3(blocks), dim3(256), 0, st, pred, target, dpred, n, g, scratch);
  else hipLaunchKernelGGL(l1_sum_grad_kernel<1>, dim3(blocks), dim3(256), 0, st, pred, target, dpred, n, g, scratch);
  hipLaunchKernelGGL(l1_sum_final_kernel, dim3(1), dim3(64), 0, st, scratch, blocks, sum);
  return check_launch("ldmk_l1_sum_grad");
}
