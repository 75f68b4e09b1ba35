// The diffusion training objective of LatentDiffusion.p_losses (ddpm.py:1014-1047) in one pass over the UNet output: l1 or l2,
// the learned log-variance weighting, the VLB term, their gradient w.r.t. the prediction and w.r.t. logvar.  gfx950 only.
// The conventions of backward.hip / kl_train.hip: fp32 in and out, no float atomics, every sum kept in double in one fixed order
// (per-workgroup partials in a caller-supplied scratch, added in workgroup order by a final kernel): bitwise reproducible.
//
// pred / dpred are the trainer's channel-padded NHWC rows (n, hw, 32); target is NCHW (n, c, hw), read where it lies.  A workgroup
// walks 64-pixel tiles of one sample: the tile's c target planes are staged through LDS with 64-wide coalesced reads, then lane
// (pixel, q) handles the four channels 4q..4q+3 of its pixel with one 16-byte load and one 16-byte store.  The gradient scale of
// a sample, (l_simple_weight e^{-lv} + original_elbo_weight w) / (n per), does not depend on the sample's loss, so dpred is
// written in the pass that reduces; it is formed in double and rounded once.
#include "ldmk_common.h"

namespace ldmk {

constexpr int OBJ_BPS = 64;     // workgroups per sample at the most
constexpr int OBJ_TP = 64;      // pixels per tile
constexpr int OBJ_SCRATCH_PER_SAMPLE = OBJ_BPS + 4;   // partials, then (ls, gamma term, vlb term, dlogvar term)

__device__ __forceinline__ long long obj_timestep(const long long* t, int b, int T) {
  const long long tb = t[b];                     // an index outside [0, T) is clamped into it (no out-of-bounds table read)
  return tb < 0 ? 0 : (tb >= T ? T - 1 : tb);
}

template <bool L1>
__global__ __launch_bounds__(256) void diffusion_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                             const long long* __restrict__ t, const float* __restrict__ logvar,
                                                             const float* __restrict__ lvlb, float* __restrict__ dpred, int c, int hw,
                                                             int T, double lsw, double oew, double count,
                                                             double* __restrict__ partial) {
  __shared__ float tile[32][OBJ_TP + 1];
  __shared__ double red[4];
  const int b = blockIdx.y;
  float g = 0.f;
  if (dpred) {
    const long long tb = obj_timestep(t, b, T);
    const double lv = (double)logvar[tb], w = (double)lvlb[tb];
    g = (float)((lsw * exp(-lv) + oew * w) / count * (L1 ? 1.0 : 2.0));
  }
  const int q = threadIdx.x & 7, pl = threadIdx.x >> 3;      // 8 lanes of 4 channels per pixel, 32 pixels per pass
  const int ntiles = (hw + OBJ_TP - 1) / OBJ_TP;
  const float* tb_ = target + (long long)b * c * hw;
  double s = 0.0;
  for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {   // (the trip count is the workgroup's: the barriers are uniform)
    const int p0 = ti * OBJ_TP, np = hw - p0 < OBJ_TP ? hw - p0 : OBJ_TP;
    __syncthreads();
    for (int i = threadIdx.x; i < c * OBJ_TP; i += 256) {
      const int ch = i / OBJ_TP, p = i % OBJ_TP;
      if (p < np) tile[ch][p] = tb_[(long long)ch * hw + p0 + p];
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < OBJ_TP / 32; ++h) {
      const int p = pl + 32 * h;
      if (p >= np) continue;
      const long long row = ((long long)b * hw + p0 + p) * 32 + 4 * q;
      float o[4] = {0.f, 0.f, 0.f, 0.f};                      // the pad lanes stay exact zeros
      if (4 * q < c) {
        const float4 p4 = *reinterpret_cast<const float4*>(pred + row);
        const float pv[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (4 * q + k >= c) continue;
          const float d = pv[k] - tile[4 * q + k][p];
          if constexpr (L1) {
            s += (double)fabsf(d);
            o[k] = d > 0.f ? g : (d < 0.f ? -g : d * 0.f);     // sign(0) = 0 as torch.sign has it; a NaN stays a NaN
          } else {
            s += (double)d * (double)d;
            o[k] = g * d;
          }
        }
      }
      if (dpred) *reinterpret_cast<float4*>(dpred + row) = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[(long long)b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup.  Per sample, in double from the double ls_b: the terms of the three means and of dlogvar; then thread 0 adds the
// means in sample order, and entry tau of the dense dlogvar is the sum, in sample order, over the samples with t_b = tau (one
// writer per entry, zero where no sample sits).
__global__ __launch_bounds__(256) void diffusion_loss_final_kernel(const double* __restrict__ partial, double* __restrict__ terms,
                                                                   const long long* __restrict__ t, const float* __restrict__ logvar,
                                                                   const float* __restrict__ lvlb, int n, int bps, int T, double per,
                                                                   double lsw, double oew, float* __restrict__ scalars,
                                                                   float* __restrict__ ls_out, float* __restrict__ dlogvar) {
  for (int b = threadIdx.x; b < n; b += blockDim.x) {
    double s = 0.0;
    for (int i = 0; i < bps; ++i) s += partial[(long long)b * bps + i];
    const double ls = s / per;
    const long long tb = obj_timestep(t, b, T);
    const double lv = (double)logvar[tb], w = (double)lvlb[tb], e = exp(-lv);
    terms[b] = ls;
    terms[n + b] = ls * e + lv;
    terms[2 * (long long)n + b] = w * ls;
    terms[3 * (long long)n + b] = lsw / (double)n * (1.0 - ls * e);
    ls_out[b] = (float)ls;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, gm = 0.0, v = 0.0;
    for (int b = 0; b < n; ++b) {
      a += terms[b];
      gm += terms[n + b];
      v += terms[2 * (long long)n + b];
    }
    a /= (double)n; gm /= (double)n; v /= (double)n;
    scalars[0] = (float)(lsw * gm + oew * v);
    scalars[1] = (float)a;
    scalars[2] = (float)gm;
    scalars[3] = (float)v;
  }
  if (dlogvar) {
    for (int tau = threadIdx.x; tau < T; tau += blockDim.x) {
      double d = 0.0;
      for (int b = 0; b < n; ++b)
        if (obj_timestep(t, b, T) == tau) d += terms[3 * (long long)n + b];
      dlogvar[tau] = (float)d;
    }
  }
}

}  // namespace ldmk

using namespace ldmk;

extern "C" long long ldmk_diffusion_loss_scratch_elems(int n) { return n > 0 ? (long long)n * OBJ_SCRATCH_PER_SAMPLE : 0; }

extern "C" int ldmk_diffusion_loss(const float* pred, const float* target, const long long* t, const float* logvar,
                                   const float* lvlb_weights, float* dpred, float* dlogvar, float* scalars, float* ls, int n, int c,
                                   int hw, int T, int loss_type, float l_simple_weight, float original_elbo_weight, double* scratch,
                                   void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(pred && target && t && logvar && lvlb_weights && scalars && ls && scratch && n > 0 && c > 0 && hw > 0 && T > 0,
               "ldmk_diffusion_loss: bad args");
  LDMK_REQUIRE(c <= 32, "ldmk_diffusion_loss: c=%d channels above the 32 of the padded layout", c);
  LDMK_REQUIRE(n <= 65535, "ldmk_diffusion_loss: n=%d above 65535 samples", n);
  LDMK_REQUIRE(loss_type == 1 || loss_type == 2, "ldmk_diffusion_loss: loss_type=%d (1: l1, 2: l2)", loss_type);
  LDMK_REQUIRE(((uintptr_t)pred & 15) == 0 && ((uintptr_t)dpred & 15) == 0, "ldmk_diffusion_loss: pred / dpred off a 16-byte boundary");
  const int ntiles = (hw + OBJ_TP - 1) / OBJ_TP;
  const int bps = ntiles > OBJ_BPS ? OBJ_BPS : ntiles;
  const double per = (double)c * (double)hw, count = per * (double)n;
  const double lsw = (double)l_simple_weight, oew = (double)original_elbo_weight;
  const dim3 grid((unsigned)bps, (unsigned)n), block(256);
  hipStream_t st = (hipStream_t)stream;
  double* terms = scratch + (long long)n * OBJ_BPS;
  if (loss_type == 1)
    hipLaunchKernelGGL(diffusion_loss_kernel<true>, grid, block, 0, st, pred, target, t, logvar, lvlb_weights, dpred, c, hw, T, lsw,
                       oew, count, scratch);
  else
    hipLaunchKernelGGL(diffusion_loss_kernel<false>, grid, block, 0, st, pred, target, t, logvar, lvlb_weights, dpred, c, hw, T, lsw,
                       oew, count, scratch);
  hipLaunchKernelGGL(diffusion_loss_final_kernel, dim3(1), dim3(256), 0, st, scratch, terms, t, logvar, lvlb_weights, n, bps, T, per,
                     lsw, oew, scalars, ls, dlogvar);
  return check_launch("ldmk_diffusion_loss");
}
