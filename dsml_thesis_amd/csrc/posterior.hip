// KL first stage (autoencoder.py:285-342, distributions.py:24-62): the encoder's moment head and the diagonal-Gaussian
// posterior.  gfx950 only.
#include "ldmk_common.h"

namespace ldmk {

// ---------------------------------------------------------------------------------------------
// Moment head of a KL encoder: GroupNorm+SiLU (coef planes) -> 3x3 pad-1 conv cin -> C2Z (Encoder.conv_out with
// double_z, model.py:427-431,457-459) -> 1x1 conv C2Z -> c2e (quant_conv, autoencoder.py:302,326), NHWC in -> NCHW
// `moments` out, one launch.  The tiling is conv3x3_out_kernel's (small.hip): workgroup = 16x16 output pixels, the 18x18
// input tile staged through LDS in 32-channel chunks and activated ONCE per element, thread <-> pixel, wave-uniform
// weights.  A thread's C2Z accumulators walk the channels in that kernel's order (chunk, tap, channel), stay in registers
// and feed the 1x1 directly; the 1x1's <= 64 weights and both biases are read at wave-uniform addresses.  LDS: tile
// 18*18*36 floats (46656 B) + one weight chunk 9*32*WP floats (<= 9216 B) = 55872 B at C2Z = 8.
constexpr int MH_T = 16, MH_CK = 32, MH_STR = 36;
template <int C2Z>
__global__ __launch_bounds__(256) void conv3x3_moments_kernel(const float* __restrict__ x, const float* __restrict__ coef,
                                                              const float* __restrict__ w3, const float* __restrict__ b3,
                                                              const float* __restrict__ w1, const float* __restrict__ b1,
                                                              float* __restrict__ out, int n, int h, int wd, int cin,
                                                              int c2e) {
  constexpr int WP = C2Z <= 4 ? 4 : 8;                                         // weight row padded to whole float4s
  __shared__ __attribute__((aligned(16))) float tile[(MH_T + 2) * (MH_T + 2) * MH_STR];
  __shared__ __attribute__((aligned(16))) float wch[9 * MH_CK * WP];           // this chunk's weights, [tap][c][WP]
  const int tx_n = (wd + MH_T - 1) / MH_T, ty_n = (h + MH_T - 1) / MH_T;
  const int b = blockIdx.x / (tx_n * ty_n), t = blockIdx.x % (tx_n * ty_n);
  const int y0 = (t / tx_n) * MH_T, x0 = (t % tx_n) * MH_T;
  const int ty = threadIdx.x / MH_T, tx = threadIdx.x % MH_T;
  const float* sc = coef ? coef + ((long long)b * 2) * cin : nullptr;
  float acc[WP];
#pragma unroll
  for (int z = 0; z < WP; ++z) acc[z] = 0.f;
  for (int c0 = 0; c0 < cin; c0 += MH_CK) {
    __syncthreads();                                   // the previous chunk's reads are done
    for (int i = threadIdx.x; i < (MH_T + 2) * (MH_T + 2) * (MH_CK / 4); i += 256) {
      const int c4 = i % (MH_CK / 4), pix = i / (MH_CK / 4);
      const int yy = y0 + pix / (MH_T + 2) - 1, xx = x0 + pix % (MH_T + 2) - 1;
      const int c = c0 + 4 * c4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);      // zero padding applies to the ACTIVATED tensor
      if (yy >= 0 && yy < h && xx >= 0 && xx < wd && c < cin) {
        v = *reinterpret_cast<const float4*>(x + (((long long)b * h + yy) * wd + xx) * cin + c);
        if (sc) {
          const float4 s4 = *reinterpret_cast<const float4*>(sc + c), t4 = *reinterpret_cast<const float4*>(sc + cin + c);
          v.x = silu_f(fmaf(v.x, s4.x, t4.x)); v.y = silu_f(fmaf(v.y, s4.y, t4.y));
          v.z = silu_f(fmaf(v.z, s4.z, t4.z)); v.w = silu_f(fmaf(v.w, s4.w, t4.w));
        }
      }
      *reinterpret_cast<float4*>(tile + pix * MH_STR + 4 * c4) = v;
    }
    for (int i = threadIdx.x; i < 9 * MH_CK * WP; i += 256) {
      const int co = i % WP, c = (i / WP) % MH_CK, tap = i / (WP * MH_CK);
      wch[i] = (co < C2Z && c0 + c < cin) ? w3[((long long)tap * cin + c0 + c) * C2Z + co] : 0.f;
    }
    __syncthreads();
    // every lane reads the same weight address (LDS broadcast); channels beyond cin hold zero data and zero weights
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const float* tp = tile + ((ty + tap / 3) * (MH_T + 2) + tx + tap % 3) * MH_STR;
      const float4* wp = reinterpret_cast<const float4*>(wch + tap * MH_CK * WP);
#pragma unroll
      for (int c = 0; c < MH_CK; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(tp + c);
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 wa = wp[(c + q) * (WP / 4)];
          acc[0] = fmaf(vv[q], wa.x, acc[0]);
          if (C2Z > 1) acc[1] = fmaf(vv[q], wa.y, acc[1]);
          if (C2Z > 2) acc[2] = fmaf(vv[q], wa.z, acc[2]);
          if (C2Z > 3) acc[3] = fmaf(vv[q], wa.w, acc[3]);
          if constexpr (C2Z > 4) {
            const float4 wb = wp[(c + q) * 2 + 1];
            acc[4] = fmaf(vv[q], wb.x, acc[4]);
            if (C2Z > 5) acc[5] = fmaf(vv[q], wb.y, acc[5]);
            if (C2Z > 6) acc[6] = fmaf(vv[q], wb.z, acc[6]);
            if (C2Z > 7) acc[7] = fmaf(vv[q], wb.w, acc[7]);
          }
        }
      }
    }
  }
  const int oy = y0 + ty, ox = x0 + tx;
  if (oy < h && ox < wd) {
#pragma unroll
    for (int z = 0; z < C2Z; ++z) acc[z] += b3 ? b3[z] : 0.f;
    // quant_conv: out[e] = b1[e] + sum_z w1[e][z] * hz[z], z ascending
    for (int e = 0; e < c2e; ++e) {
      float m = b1 ? b1[e] : 0.f;
#pragma unroll
      for (int z = 0; z < C2Z; ++z) m = fmaf(acc[z], w1[e * C2Z + z], m);
      out[((long long)b * c2e + e) * h * wd + (long long)oy * wd + ox] = m;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// DiagonalGaussianDistribution (distributions.py:24-37) over moments (n, 2e, hw): channels [0,e) are the mean, [e,2e) the
// log-variance.  Per element: logvar = clamp(lv, -30, 20), std = exp(0.5 logvar), var = exp(logvar),
// z = scale * (mean + std * noise) (noise null: scale * mean).  Null outputs are skipped.  expf is the accurate one: the
// exponential IS the result here.  V = 4: 16-byte accesses (a sample's e*hw plane is a multiple of 4 floats, so a vector
// never straddles the mean / log-variance boundary); V = 1: the scalar form for everything else.
template <int V>
__global__ __launch_bounds__(256) void gauss_posterior_kernel(const float* __restrict__ moments, const float* __restrict__ noise,
                                                              float scale, float* __restrict__ logvar, float* __restrict__ stdo,
                                                              float* __restrict__ var, float* __restrict__ z, long long plane,
                                                              long long total) {
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V; i < total; i += (long long)gridDim.x * blockDim.x * V) {
    const long long b = i / plane, r = i - b * plane;
    const float* mp = moments + b * 2 * plane + r;
    float mean[V], lv[V], nz[V];
    if constexpr (V == 4) {
      const float4 m4 = *reinterpret_cast<const float4*>(mp), l4 = *reinterpret_cast<const float4*>(mp + plane);
      mean[0] = m4.x; mean[1] = m4.y; mean[2] = m4.z; mean[3] = m4.w;
      lv[0] = l4.x; lv[1] = l4.y; lv[2] = l4.z; lv[3] = l4.w;
      if (z && noise) {
        const float4 n4 = *reinterpret_cast<const float4*>(noise + i);
        nz[0] = n4.x; nz[1] = n4.y; nz[2] = n4.z; nz[3] = n4.w;
      }
    } else {
      mean[0] = mp[0];
      lv[0] = mp[plane];
      if (z && noise) nz[0] = noise[i];
    }
    float sd[V], vr[V], zz[V];
    const bool need_std = stdo || (z && noise);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      lv[k] = fminf(fmaxf(lv[k], -30.0f), 20.0f);
      sd[k] = need_std ? expf(0.5f * lv[k]) : 0.f;
      vr[k] = var ? expf(lv[k]) : 0.f;
      zz[k] = (z && noise) ? scale * fmaf(sd[k], nz[k], mean[k]) : scale * mean[k];
    }
    if constexpr (V == 4) {
      if (logvar) *reinterpret_cast<float4*>(logvar + i) = make_float4(lv[0], lv[1], lv[2], lv[3]);
      if (stdo) *reinterpret_cast<float4*>(stdo + i) = make_float4(sd[0], sd[1], sd[2], sd[3]);
      if (var) *reinterpret_cast<float4*>(var + i) = make_float4(vr[0], vr[1], vr[2], vr[3]);
      if (z) *reinterpret_cast<float4*>(z + i) = make_float4(zz[0], zz[1], zz[2], zz[3]);
    } else {
      if (logvar) logvar[i] = lv[0];
      if (stdo) stdo[i] = sd[0];
      if (var) var[i] = vr[0];
      if (z) z[i] = zz[0];
    }
  }
}

}  // namespace ldmk

using namespace ldmk;

extern "C" int ldmk_conv3x3_moments(const float* x, const float* coef, const float* w3, const float* b3, const float* w1,
                                    const float* b1, float* out, int n, int h, int w_, int cin, int c2z, int c2e,
                                    void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(c2z >= 2 && c2z <= 8 && c2z % 2 == 0, "ldmk_conv3x3_moments: c2z=%d must be one of 2, 4, 6, 8 (z_channels <= 4)", c2z);
  LDMK_REQUIRE(c2e >= 2 && c2e <= 8 && c2e % 2 == 0, "ldmk_conv3x3_moments: c2e=%d must be one of 2, 4, 6, 8 (embed_dim <= 4)", c2e);
  LDMK_REQUIRE(cin > 0 && cin % 4 == 0, "ldmk_conv3x3_moments: cin=%d must be a positive multiple of 4", cin);
  LDMK_REQUIRE(x && w3 && w1 && out && n > 0 && h > 0 && w_ > 0, "ldmk_conv3x3_moments: bad args");
  const long long blocks = (long long)n * ((h + MH_T - 1) / MH_T) * ((w_ + MH_T - 1) / MH_T);
  LDMK_REQUIRE(blocks < (1LL << 31), "ldmk_conv3x3_moments: too many tiles");
  const dim3 grid((unsigned)blocks), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (c2z) {
    case 2: hipLaunchKernelGGL(conv3x3_moments_kernel<2>, grid, block, 0, st, x, coef, w3, b3, w1, b1, out, n, h, w_, cin, c2e); break;
    case 4: hipLaunchKernelGGL(conv3x3_moments_kernel<4>, grid, block, 0, st, x, coef, w3, b3, w1, b1, out, n, h, w_, cin, c2e); break;
    case 6: hipLaunchKernelGGL(conv3x3_moments_kernel<6>, grid, block, 0, st, x, coef, w3, b3, w1, b1, out, n, h, w_, cin, c2e); break;
    default: hipLaunchKernelGGL(conv3x3_moments_kernel<8>, grid, block, 0, st, x, coef, w3, b3, w1, b1, out, n, h, w_, cin, c2e); break;
  }
  return check_launch("ldmk_conv3x3_moments");
}

extern "C" int ldmk_gauss_posterior(const float* moments, const float* noise, float scale, float* logvar, float* std_,
                                    float* var, float* z, int n, int e, int hw, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(moments && n > 0 && e > 0 && hw > 0, "ldmk_gauss_posterior: bad args");
  LDMK_REQUIRE(logvar || std_ || var || z, "ldmk_gauss_posterior: no output requested");
  LDMK_REQUIRE(!noise || z, "ldmk_gauss_posterior: noise without z");
  const long long plane = (long long)e * hw, total = plane * n;
  auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  const bool vec = plane % 4 == 0 && al(moments) && al(noise) && al(logvar) && al(std_) && al(var) && al(z);
  long long g = ((vec ? total / 4 : total) + 255) / 256;
  if (g > 4096) g = 4096;
  const dim3 grid((unsigned)g), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(gauss_posterior_kernel<4>, grid, block, 0, st, moments, noise, scale, logvar, std_, var, z, plane, total);
  else
    hipLaunchKernelGGL(gauss_posterior_kernel<1>, grid, block, 0, st, moments, noise, scale, logvar, std_, var, z, plane, total);
  return check_launch("ldmk_gauss_posterior");
}
