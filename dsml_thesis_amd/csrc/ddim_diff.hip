// The differentiable DDIM update and its transpose (ddim2cond.py:272-308 differentiable_p_sample_ddim, eta >= 0; the
// talking-face fine-tune, ddpm2condtune.py:1026-1032, runs 8 of them at eta = 1 through the UNet training engine).
// The update is linear in x, eps and the drawn noise, so one elementwise launch each way replaces the chains of
// ldmk_axpy / concat / pad launches it was first built from.  fp32 throughout; the coefficients are host floats.
#include "ldmk_common.h"

namespace ldmk {

static inline int dd_grid(long long items) {
  long long g = (items + 255) / 256;
  return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

// One element of the forward update.  The order of operations is part of the contract (include/ldmk.h):
//   e   = fma(scale, e_c, (1 - scale) * e_u)           (guidance on; e = eps otherwise)
//   t   = fma(sigma, z, cx * x)                         (noise given; t = cx * x otherwise)
//   out = fma(ce, e, t)
__device__ __forceinline__ float dd_fwd1(float x, float eu, float ec, float z, bool guided, bool noisy, float cx, float ce,
                                         float sigma, float scale, float oms) {
  const float e = guided ? fmaf(scale, ec, oms * eu) : eu;
  const float t = noisy ? fmaf(sigma, z, cx * x) : cx * x;
  return fmaf(ce, e, t);
}

// x / out are `nruns` runs of `run` contiguous floats, `x_rs` / `out_rs` floats apart (one run when both tensors are
// plain (n,C,H,W); one run per sample when either sits in channels [0,C) of a wider NCHW buffer); eps halves and noise
// are contiguous.  out may alias x (every element is read and written by the same thread).  VEC: every run starts on
// a 16-byte boundary in all five tensors -- float4 body, scalar tail of run % 4 elements.
template <bool VEC>
__global__ __launch_bounds__(256) void ddim_diff_fwd_kernel(const float* x, long long x_rs, const float* __restrict__ eu,
                                                            const float* __restrict__ ec, const float* __restrict__ z, float* out,
                                                            long long out_rs, long long run, long long nruns, float cx, float ce,
                                                            float sigma, float scale) {
  const bool guided = ec != nullptr, noisy = z != nullptr;
  const float oms = 1.0f - scale;
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long long)gridDim.x * blockDim.x;
  const long long quads = VEC ? run / 4 : 0;
  if (VEC) {
    for (long long i = tid; i < nruns * quads; i += nth) {
      const long long r = i / quads, k = (i - r * quads) * 4, c = r * run + k;
      const float4 xv = *reinterpret_cast<const float4*>(x + r * x_rs + k);
      const float4 uv = *reinterpret_cast<const float4*>(eu + c);
      const float4 cv = guided ? *reinterpret_cast<const float4*>(ec + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 zv = noisy ? *reinterpret_cast<const float4*>(z + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 o;
      o.x = dd_fwd1(xv.x, uv.x, cv.x, zv.x, guided, noisy, cx, ce, sigma, scale, oms);
      o.y = dd_fwd1(xv.y, uv.y, cv.y, zv.y, guided, noisy, cx, ce, sigma, scale, oms);
      o.z = dd_fwd1(xv.z, uv.z, cv.z, zv.z, guided, noisy, cx, ce, sigma, scale, oms);
      o.w = dd_fwd1(xv.w, uv.w, cv.w, zv.w, guided, noisy, cx, ce, sigma, scale, oms);
      *reinterpret_cast<float4*>(out + r * out_rs + k) = o;
    }
  }
  const long long tail = run - quads * 4;
  for (long long j = tid; j < nruns * tail; j += nth) {
    const long long r = j / tail, k = quads * 4 + (j - r * tail), c = r * run + k;
    out[r * out_rs + k] = dd_fwd1(x[r * x_rs + k], eu[c], guided ? ec[c] : 0.f, noisy ? z[c] : 0.f, guided, noisy, cx, ce, sigma,
                                  scale, oms);
  }
}

// Transpose.  One thread per (sample, pixel, 4 padded channels) of the NHWC output gradient: for a real channel c < C
//   v = fma(cx, dx_prev, dxin[b]) (+ dxin[n + b] under guidance)        (v = cx * dx_prev without dxin)
// is written to dx (NCHW) and scaled into deps: ce * v, or the two rows ce * (1 - scale) * v and ce * scale * v; the
// padded channels are written as zeros.  dx may alias dx_prev.  VEC: deps is 16-byte aligned (float4 stores).
// The thread order follows the NHWC output (channel quad fastest), because with cpad = 32 against C = 3 or 4 the output
// gradient is nine tenths of the bytes moved and its stores are then contiguous float4s.  The NCHW reads of dx_prev / dxin
// are the price: lanes that share a pixel read channels 4*hw floats apart, and with C <= 4 only one thread in cpad / 4 has
// a real channel at all -- the others store zeros.  Transposing through LDS would fix the reads; at n*C*hw of a few
// thousand floats the whole launch is latency, so it is not done.
template <bool VEC>
__global__ __launch_bounds__(256) void ddim_diff_bwd_kernel(const float* dx_prev, const float* __restrict__ dxin, int cin, float* dx,
                                                            float* __restrict__ deps, int cpad, int n, int C, int hw, float cx,
                                                            float ce, float scale, int guided) {
  const int Q = cpad / 4;
  const long long total = (long long)n * hw * Q;
  const float wu = guided ? ce * (1.0f - scale) : ce, wc = ce * scale;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int q = (int)(i % Q);
    const long long bp = i / Q;
    const int p = (int)(bp % hw), b = (int)(bp / hw);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = 4 * q + j;
      v[j] = 0.f;
      if (c < C) {
        const long long o = ((long long)b * C + c) * hw + p;
        const float g = dx_prev[o];
        float a = cx * g;
        if (dxin) {
          a = fmaf(cx, g, dxin[((long long)b * cin + c) * hw + p]);
          if (guided) a += dxin[((long long)(b + n) * cin + c) * hw + p];
        }
        if (dx) dx[o] = a;
        v[j] = a;
      }
    }
    if (!deps) continue;
    float* du = deps + ((long long)b * hw + p) * cpad + 4 * q;
    float* dc = deps + ((long long)(b + n) * hw + p) * cpad + 4 * q;
    if (VEC) {
      *reinterpret_cast<float4*>(du) = make_float4(wu * v[0], wu * v[1], wu * v[2], wu * v[3]);
      if (guided) *reinterpret_cast<float4*>(dc) = make_float4(wc * v[0], wc * v[1], wc * v[2], wc * v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        du[j] = wu * v[j];
        if (guided) dc[j] = wc * v[j];
      }
    }
  }
}

static inline bool dd_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace ldmk

using namespace ldmk;

extern "C" int ldmk_ddim_diff_fwd(const float* x, int x_channels, const float* eps, const float* noise, float* out,
                                  int out_channels, int n, int C, int hw, float cx, float ce, float sigma, float scale, int guided,
                                  void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(x && eps && out && n > 0 && C > 0 && hw > 0, "ldmk_ddim_diff_fwd: bad args");
  LDMK_REQUIRE(x_channels >= C && out_channels >= C, "ldmk_ddim_diff_fwd: x_channels=%d / out_channels=%d below C=%d", x_channels,
               out_channels, C);
  LDMK_REQUIRE(noise || sigma == 0.f, "ldmk_ddim_diff_fwd: sigma != 0 needs the noise tensor");
  const long long per = (long long)C * hw;
  const bool flat = x_channels == C && out_channels == C;
  const long long nruns = flat ? 1 : n, run = flat ? (long long)n * per : per;
  const long long x_rs = (long long)x_channels * hw, out_rs = (long long)out_channels * hw;
  const float* ec = guided ? eps + (long long)n * per : nullptr;
  bool vec = dd_al16(x) && dd_al16(eps) && dd_al16(out) && (!ec || dd_al16(ec)) && (!noise || dd_al16(noise));
  if (!flat) vec = vec && run % 4 == 0 && x_rs % 4 == 0 && out_rs % 4 == 0;
  const long long items = vec ? nruns * (run / 4) + nruns * (run % 4) : nruns * run;
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(ddim_diff_fwd_kernel<true>, dim3(dd_grid(items)), dim3(256), 0, st, x, x_rs, eps, ec, noise, out, out_rs, run,
                       nruns, cx, ce, sigma, scale);
  else
    hipLaunchKernelGGL(ddim_diff_fwd_kernel<false>, dim3(dd_grid(items)), dim3(256), 0, st, x, x_rs, eps, ec, noise, out, out_rs, run,
                       nruns, cx, ce, sigma, scale);
  return check_launch("ldmk_ddim_diff_fwd");
}

extern "C" int ldmk_ddim_diff_bwd(const float* dx_prev, const float* dxin, int in_channels, float* dx, float* deps, int cpad, int n,
                                  int C, int hw, float cx, float ce, float scale, int guided, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(dx_prev && (dx || deps) && n > 0 && C > 0 && hw > 0, "ldmk_ddim_diff_bwd: bad args");
  LDMK_REQUIRE(!dxin || in_channels >= C, "ldmk_ddim_diff_bwd: in_channels=%d below C=%d", in_channels, C);
  LDMK_REQUIRE(cpad >= C && cpad % 4 == 0, "ldmk_ddim_diff_bwd: cpad=%d must be a multiple of 4 and >= C=%d", cpad, C);
  const long long total = (long long)n * hw * (cpad / 4);
  hipStream_t st = (hipStream_t)stream;
  if (!deps || dd_al16(deps))
    hipLaunchKernelGGL(ddim_diff_bwd_kernel<true>, dim3(dd_grid(total)), dim3(256), 0, st, dx_prev, dxin, in_channels, dx, deps, cpad,
                       n, C, hw, cx, ce, scale, guided);
  else
    hipLaunchKernelGGL(ddim_diff_bwd_kernel<false>, dim3(dd_grid(total)), dim3(256), 0, st, dx_prev, dxin, in_channels, dx, deps, cpad,
                       n, C, hw, cx, ce, scale, guided);
  return check_launch("ldmk_ddim_diff_bwd");
}
