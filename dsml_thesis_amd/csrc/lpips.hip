// LPIPS over VGG16 (taming/modules/losses/lpips.py): the memory-bound kernels around the thirteen 3x3 convolutions, value and
// image gradient.  The twelve inner convolutions and their data gradients run on ldmk_igemm; the network is frozen, so there
// is no weight gradient.  gfx950 only.  The conventions of vq_train.hip / kl_train.hip / classifier.hip: fp32 in and out, no
// float atomics, every cross-pixel sum kept in double in one fixed order (per-workgroup partials in a caller-supplied scratch,
// added in workgroup order by a final kernel), so every output is bitwise reproducible; arguments are validated before any
// launch.  Activations are NHWC; the image and its gradient are NCHW.
//
// One divergence from torch autograd, in ldmk_lpips_layer_bwd: a feature vector that is all zero (norm 0) gives 0/0 = NaN in
// the backward of torch.sqrt; here the norm term contributes 0 there and the result is the finite r * a (see the kernel).
#include "ldmk_common.h"

namespace ldmk {

constexpr int LP_BPS = 64;          // workgroups per sample at the most in ldmk_lpips_layer (scratch: n * LP_BPS doubles)
constexpr int LP_BLOCKS = 2048;    // workgroups of a grid-stride kernel at the most: 8 per CU, 32 waves per CU -- full occupancy
constexpr int LP_CONV_BLOCKS = 16384;   // ... of the two boundary-convolution kernels: measured 27 % (128^2) to 36 % (256^2) faster than at 2048
constexpr float LP_EPS = 1e-10f;    // normalize_tensor's eps, added OUTSIDE the square root

inline unsigned lp_grid(long long items, int per_block, long long cap) {
  const long long g = (items + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---------------------------------------------------------------------------------------------
// conv1_1 with the ScalingLayer on load: x (n,3,h,w) NCHW, wt (64,3,3,3) OIHW as torch stores it, out (n,h,w,64) NHWC =
// relu(bias + sum_{c,ky,kx} wt[o][c][ky][kx] * s(c, y+ky-1, x+kx-1)), s = (x - shift[c]) / scale[c] inside the image and 0
// outside (the zero padding is of the SCALED tensor, so the shift is not folded into the bias).  One wave per pixel, lane = output
// channel: lanes 0..26 load and scale one tap each and the wave reads them by lane index (27 divisions per pixel, not 27 per
// output), the 64 outputs are one 256-byte store; each lane keeps its 27 weights in registers.
__global__ __launch_bounds__(256) void lpips_conv_in_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                            const float* __restrict__ bias, const float* __restrict__ shift,
                                                            const float* __restrict__ scale, float* __restrict__ out, int h, int w,
                                                            long long pixels) {
  const int o = threadIdx.x & 63;
  float wr[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) wr[k] = wt[o * 27 + k];
  const float b = bias[o];
  const int tc = o < 27 ? o / 9 : 0, tk = o % 9;
  const float tsh = shift[tc], tsc = scale[tc];
  const long long plane = (long long)h * w;
  for (long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); p < pixels; p += (long long)gridDim.x * 4) {
    const long long bi = p / plane;
    const int r = (int)(p - bi * plane), py = r / w, px = r - py * w;
    const float* xb = x + bi * 3 * plane;
    float s = 0.f;                                      // lane k < 27 loads and scales tap k = c * 9 + ky * 3 + kx once for the wave
    if (o < 27) {
      const int iy = py + tk / 3 - 1, ix = px + tk % 3 - 1;
      if (iy >= 0 && iy < h && ix >= 0 && ix < w) s = (xb[tc * plane + (long long)iy * w + ix] - tsh) / tsc;
    }
    float acc = b;
#pragma unroll
    for (int k = 0; k < 27; ++k) acc = fmaf(wr[k], __shfl(s, k, 64), acc);
    out[p * 64 + o] = fmaxf(acc, 0.f);
  }
}

// Its data gradient: dy (n,h,w,64), y the saved post-ReLU output (the mask y > 0) -> dx (n,3,h,w) NCHW,
//   dx[c][iy][ix] = (sum_{ky,kx} sum_o [y > 0] dy[iy-ky+1][ix-kx+1][o] wt[o][c][ky][kx]) / scale[c].
// One wave per input pixel, lane = output channel: nine coalesced 256-byte reads of dy and y, three partial sums per lane, three
// wave butterflies; lanes 0..2 store channel 0..2.  K = 27: not a matrix-core kernel.
__global__ __launch_bounds__(256) void lpips_conv_in_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                                const float* __restrict__ wt, const float* __restrict__ scale,
                                                                float* __restrict__ dx, int h, int w, long long pixels) {
  const int o = threadIdx.x & 63;
  float wr[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) wr[k] = wt[o * 27 + k];
  const long long plane = (long long)h * w;
  for (long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); p < pixels; p += (long long)gridDim.x * 4) {
    const long long bi = p / plane;
    const int r = (int)(p - bi * plane), iy = r / w, ix = r - iy * w;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int oy = iy - ky + 1;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ox = ix - kx + 1;
        if (oy >= 0 && oy < h && ox >= 0 && ox < w) {             // (wave-uniform)
          const long long q = ((bi * plane + (long long)oy * w + ox) << 6) + o;
          const float g = y[q] > 0.f ? dy[q] : 0.f;
          s0 = fmaf(g, wr[ky * 3 + kx], s0);
          s1 = fmaf(g, wr[9 + ky * 3 + kx], s1);
          s2 = fmaf(g, wr[18 + ky * 3 + kx], s2);
        }
      }
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (o < 3) dx[(bi * 3 + o) * plane + r] = (o == 0 ? s0 : (o == 1 ? s1 : s2)) / scale[o];
  }
}

// ---------------------------------------------------------------------------------------------
// ReLU then MaxPool2d(2, 2) of an NHWC map x (n,h,w,C): pooled (n, h/2, w/2, C), and -- relu_out non-null -- the full-resolution
// post-ReLU map (the LPIPS tap), which may be x itself: a thread reads the up to four pixels of its window before it writes
// them, and no other thread touches them.  Windows cover ceil(h/2) x ceil(w/2): the partial ones of an odd trailing row or column
// only write relu_out.  The maximum scans the window in row-major order with torch's rule (v > m, or v a NaN).
template <int V>
struct lp_vec {
  float v[V];
};
template <int V>
__device__ __forceinline__ lp_vec<V> lp_load(const float* p) {
  lp_vec<V> r;
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else if constexpr (V == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    r.v[0] = t.x; r.v[1] = t.y;
  } else {
    r.v[0] = p[0];
  }
  return r;
}
template <int V>
__device__ __forceinline__ void lp_store(float* p, const lp_vec<V>& r) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else if constexpr (V == 2) *reinterpret_cast<float2*>(p) = make_float2(r.v[0], r.v[1]);
  else p[0] = r.v[0];
}

template <int V>
__global__ __launch_bounds__(256) void relu_maxpool2_kernel(const float* x, float* relu_out, float* __restrict__ pooled, int h,
                                                            int w, int c, long long total) {
  const int cv = c / V, wh = (h + 1) >> 1, ww = (w + 1) >> 1, ph = h >> 1, pw = w >> 1;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int k = (int)(i % cv) * V;
    long long t = i / cv;
    const int wx = (int)(t % ww);
    t /= ww;
    const int wy = (int)(t % wh);
    const long long bi = t / wh;
    lp_vec<V> m;
    bool first = true;
#pragma unroll
    for (int dyy = 0; dyy < 2; ++dyy)
#pragma unroll
      for (int dxx = 0; dxx < 2; ++dxx) {
        const int yy = 2 * wy + dyy, xx = 2 * wx + dxx;
        if (yy < h && xx < w) {
          const long long q = ((bi * h + yy) * w + xx) * c + k;
          lp_vec<V> v = lp_load<V>(x + q);
#pragma unroll
          for (int e = 0; e < V; ++e) {
            v.v[e] = v.v[e] > 0.f ? v.v[e] : (v.v[e] != v.v[e] ? v.v[e] : 0.f);       // relu; a NaN stays one
            if (first || v.v[e] > m.v[e] || v.v[e] != v.v[e]) m.v[e] = v.v[e];
          }
          first = false;
          if (relu_out) lp_store<V>(relu_out + q, v);
        }
      }
    if (wy < ph && wx < pw) lp_store<V>(pooled + ((bi * ph + wy) * pw + wx) * c + k, m);
  }
}

// Backward of the pair: x (n,h,w,C) is the pre-activation map or the post-ReLU one (relu is idempotent: the same argmax and the same
// mask), dy (n, h/2, w/2, C) -> dx (n,h,w,C), EVERY element written: dy at the first maximum of relu(x) in row-major window order
// where x > 0 there, 0 everywhere else -- the other three pixels, a window whose maximum is 0 (the pool hands dy to its first
// pixel, the ReLU mask then zeroes it), and a dropped odd row or column.
template <int V>
__global__ __launch_bounds__(256) void relu_maxpool2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                float* __restrict__ dx, int h, int w, int c, long long total) {
  const int cv = c / V, wh = (h + 1) >> 1, ww = (w + 1) >> 1, ph = h >> 1, pw = w >> 1;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int k = (int)(i % cv) * V;
    long long t = i / cv;
    const int wx = (int)(t % ww);
    t /= ww;
    const int wy = (int)(t % wh);
    const long long bi = t / wh;
    const bool whole = wy < ph && wx < pw;
    lp_vec<V> v[4], g;
    int arg[V];
    if (whole) {
      g = lp_load<V>(dy + ((bi * ph + wy) * pw + wx) * c + k);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = lp_load<V>(x + ((bi * h + 2 * wy + (j >> 1)) * w + 2 * wx + (j & 1)) * c + k);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        float m = fmaxf(v[0].v[e], 0.f);
        if (v[0].v[e] != v[0].v[e]) m = v[0].v[e];
        arg[e] = 0;
#pragma unroll
        for (int j = 1; j < 4; ++j) {
          const float r = v[j].v[e] > 0.f ? v[j].v[e] : (v[j].v[e] != v[j].v[e] ? v[j].v[e] : 0.f);
          if (r > m || r != r) { m = r; arg[e] = j; }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int yy = 2 * wy + (j >> 1), xx = 2 * wx + (j & 1);
      if (yy < h && xx < w) {
        lp_vec<V> o;
#pragma unroll
        for (int e = 0; e < V; ++e) o.v[e] = (whole && arg[e] == j && v[j].v[e] > 0.f) ? g.v[e] : 0.f;
        lp_store<V>(dx + ((bi * h + yy) * w + xx) * c + k, o);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// One LPIPS layer.  f0, f1 (n, hw, C) NHWC taps, lin (C,) the 1x1 weight.  Per pixel, one wave (C / 64 = VPL floats per lane, as
// 16-byte loads from VPL = 4 on: lane l holds channels [j * 256 + 4 l, + 4) of chunk j):
//   n_i = sqrt(sum_c f_i^2),  u_i = f_i / (n_i + 1e-10),  s = sum_c lin_c (u0_c - u1_c)^2          (three wave butterflies, fp32)
// Workgroup (x, b) walks sample b's pixels with stride 4 gridDim.x and adds its s in double: partial[b][x].
template <int VPL>
struct lp_row {
  static constexpr int W = VPL < 4 ? VPL : 4, CH = VPL / W;
  float v[VPL];
  __device__ __forceinline__ void load(const float* p, int lane) {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      const lp_vec<W> t = lp_load<W>(p + j * 64 * W + lane * W);
#pragma unroll
      for (int e = 0; e < W; ++e) v[j * W + e] = t.v[e];
    }
  }
  __device__ __forceinline__ void store(float* p, int lane) const {
#pragma unroll
    for (int j = 0; j < CH; ++j) {
      lp_vec<W> t;
#pragma unroll
      for (int e = 0; e < W; ++e) t.v[e] = v[j * W + e];
      lp_store<W>(p + j * 64 * W + lane * W, t);
    }
  }
  __device__ __forceinline__ float sumsq() const {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < VPL; ++e) s = fmaf(v[e], v[e], s);
    return wave_sum(s);
  }
};

template <int VPL>
__global__ __launch_bounds__(256) void lpips_layer_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                          const float* __restrict__ lin, int hw, double* __restrict__ partial) {
#pragma clang fp contract(off)      // u0 and u1 are each rounded before they are subtracted: identical taps give an exact 0
  constexpr int C = 64 * VPL;
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long b = blockIdx.y;
  lp_row<VPL> wl, a, c;
  wl.load(lin, lane);
  double sum = 0.0;
  for (int p = blockIdx.x * 4 + wv; p < hw; p += gridDim.x * 4) {
    a.load(f0 + (b * hw + p) * C, lane);
    c.load(f1 + (b * hw + p) * C, lane);
    const float r0 = 1.0f / (sqrtf(a.sumsq()) + LP_EPS), r1 = 1.0f / (sqrtf(c.sumsq()) + LP_EPS);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < VPL; ++e) {
      const float d = a.v[e] * r0 - c.v[e] * r1;
      s = fmaf(wl.v[e] * d, d, s);
    }
    sum += (double)wave_sum(s);
  }
  if (lane == 0) red[wv] = sum;
  __syncthreads();
  if (threadIdx.x == 0) partial[b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// res[b] (+)= (sum of the sample's partials, in workgroup order) / hw, rounded to fp32 once; accumulate: added to what res holds
// (the reference adds the five layers in order, val += res[l])
__global__ void lpips_layer_final_kernel(const double* __restrict__ partial, int n, int bps, int hw, int accumulate,
                                         float* __restrict__ res) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  double s = 0.0;
  for (int i = 0; i < bps; ++i) s += partial[(long long)b * bps + i];
  const float r = (float)(s / (double)hw);
  res[b] = accumulate ? res[b] + r : r;
}

// The gradient with respect to fa, the first of the two taps (the layer is symmetric: the other branch is the call with the taps
// swapped, which flips the sign of d).  With g[b] = dL / dres[b], ua = fa / (na + eps), ub likewise:
//   a_c  = 2 lin_c (ua_c - ub_c) g[b] / hw,      r = 1 / (na + eps)
//   dfa_k = r a_k - fa_k (sum_c a_c fa_c) / (na (na + eps)^2)
// na = 0 (an all-zero vector; torch autograd: NaN from 0/0 in sqrt's backward): the second term is taken as 0, dfa = r a, finite.
// relu_mask: the tap is a post-ReLU map and the gradient wanted is the pre-activation's, dfa_k = 0 where fa_k <= 0.
// accumulate: dfa is added to what df holds (the gradient that came down from the deeper slice) -- one add per element.
template <int VPL>
__global__ __launch_bounds__(256) void lpips_layer_bwd_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                              const float* __restrict__ lin, const float* __restrict__ g,
                                                              float* __restrict__ df, int hw, long long pixels, int relu_mask,
                                                              int accumulate) {
#pragma clang fp contract(off)      // as in the forward; the fused multiply-adds below are the explicit fmaf calls only
  constexpr int C = 64 * VPL;
  const int lane = threadIdx.x & 63;
  lp_row<VPL> wl, a, c, o;
  wl.load(lin, lane);
  const float inv_hw = 1.0f / (float)hw;
  for (long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); p < pixels; p += (long long)gridDim.x * 4) {
    a.load(fa + p * C, lane);
    c.load(fb + p * C, lane);
    const float na = sqrtf(a.sumsq()), nb = sqrtf(c.sumsq());
    const float r = 1.0f / (na + LP_EPS), rb = 1.0f / (nb + LP_EPS);
    const float gs = 2.0f * g[p / hw] * inv_hw;
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < VPL; ++e) {
      o.v[e] = wl.v[e] * (a.v[e] * r - c.v[e] * rb) * gs;           // a_c
      dot = fmaf(o.v[e], a.v[e], dot);
    }
    dot = wave_sum(dot);
    const float q = na > 0.f ? dot * (r * r) / na : 0.f;
    if (accumulate) c.load(df + p * C, lane);
#pragma unroll
    for (int e = 0; e < VPL; ++e) {
      float v = fmaf(-a.v[e], q, r * o.v[e]);
      if (relu_mask && !(a.v[e] > 0.f)) v = 0.f;
      o.v[e] = accumulate ? c.v[e] + v : v;
    }
    o.store(df + p * C, lane);
  }
}

}  // namespace ldmk

using namespace ldmk;

static inline bool lp_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline bool lp_chan_ok(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }

extern "C" int ldmk_lpips_conv_in(const float* x, const float* wt, const float* bias, const float* shift, const float* scale,
                                  float* out, int n, int h, int w, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(x && wt && bias && shift && scale && out && n > 0 && h > 0 && w > 0, "ldmk_lpips_conv_in: bad args");
  const long long pixels = (long long)n * h * w;
  hipLaunchKernelGGL(lpips_conv_in_kernel, dim3(lp_grid(pixels, 4, LP_CONV_BLOCKS)), dim3(256), 0, (hipStream_t)stream, x, wt, bias, shift,
                     scale, out, h, w, pixels);
  return check_launch("ldmk_lpips_conv_in");
}

extern "C" int ldmk_lpips_conv_in_bwd(const float* dy, const float* y, const float* wt, const float* scale, float* dx, int n, int h,
                                      int w, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(dy && y && wt && scale && dx && n > 0 && h > 0 && w > 0, "ldmk_lpips_conv_in_bwd: bad args");
  const long long pixels = (long long)n * h * w;
  hipLaunchKernelGGL(lpips_conv_in_bwd_kernel, dim3(lp_grid(pixels, 4, LP_CONV_BLOCKS)), dim3(256), 0, (hipStream_t)stream, dy, y, wt, scale,
                     dx, h, w, pixels);
  return check_launch("ldmk_lpips_conv_in_bwd");
}

extern "C" int ldmk_relu_maxpool2(const float* x, float* relu_out, float* pooled, int n, int h, int w, int c, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(x && pooled && n > 0 && c > 0, "ldmk_relu_maxpool2: bad args");
  LDMK_REQUIRE(h >= 2 && w >= 2, "ldmk_relu_maxpool2: h=%d, w=%d: a 2x2 window needs 2 rows and 2 columns", h, w);
  const bool vec = c % 4 == 0 && lp_al16(x) && lp_al16(relu_out) && lp_al16(pooled);
  const long long total = (long long)n * ((h + 1) / 2) * ((w + 1) / 2) * (vec ? c / 4 : c);
  const dim3 grid(lp_grid(total, 256, LP_BLOCKS)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(relu_maxpool2_kernel<4>, grid, block, 0, st, x, relu_out, pooled, h, w, c, total);
  else hipLaunchKernelGGL(relu_maxpool2_kernel<1>, grid, block, 0, st, x, relu_out, pooled, h, w, c, total);
  return check_launch("ldmk_relu_maxpool2");
}

extern "C" int ldmk_relu_maxpool2_bwd(const float* x, const float* dy, float* dx, int n, int h, int w, int c, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(x && dy && dx && n > 0 && c > 0, "ldmk_relu_maxpool2_bwd: bad args");
  LDMK_REQUIRE(h >= 2 && w >= 2, "ldmk_relu_maxpool2_bwd: h=%d, w=%d: a 2x2 window needs 2 rows and 2 columns", h, w);
  LDMK_REQUIRE(x != dx, "ldmk_relu_maxpool2_bwd: dx must not be x");
  const bool vec = c % 4 == 0 && lp_al16(x) && lp_al16(dy) && lp_al16(dx);
  const long long total = (long long)n * ((h + 1) / 2) * ((w + 1) / 2) * (vec ? c / 4 : c);
  const dim3 grid(lp_grid(total, 256, LP_BLOCKS)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(relu_maxpool2_bwd_kernel<4>, grid, block, 0, st, x, dy, dx, h, w, c, total);
  else hipLaunchKernelGGL(relu_maxpool2_bwd_kernel<1>, grid, block, 0, st, x, dy, dx, h, w, c, total);
  return check_launch("ldmk_relu_maxpool2_bwd");
}

extern "C" int ldmk_lpips_layer(const float* f0, const float* f1, const float* lin, float* res, int accumulate, int n, int hw, int c,
                                double* scratch, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(f0 && f1 && lin && res && scratch && n > 0 && hw > 0, "ldmk_lpips_layer: bad args");
  LDMK_REQUIRE(lp_chan_ok(c), "ldmk_lpips_layer: C=%d is not one of 64, 128, 256, 512", c);
  LDMK_REQUIRE(n <= 65535, "ldmk_lpips_layer: n=%d above 65535 samples", n);
  LDMK_REQUIRE(lp_al16(f0) && lp_al16(f1) && lp_al16(lin), "ldmk_lpips_layer: the taps and the weight must be 16-byte aligned");
  const int bps = (int)lp_grid(hw, 4, LP_BPS);
  const dim3 grid((unsigned)bps, (unsigned)n), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (c) {
    case 64: hipLaunchKernelGGL(lpips_layer_kernel<1>, grid, block, 0, st, f0, f1, lin, hw, scratch); break;
    case 128: hipLaunchKernelGGL(lpips_layer_kernel<2>, grid, block, 0, st, f0, f1, lin, hw, scratch); break;
    case 256: hipLaunchKernelGGL(lpips_layer_kernel<4>, grid, block, 0, st, f0, f1, lin, hw, scratch); break;
    default: hipLaunchKernelGGL(lpips_layer_kernel<8>, grid, block, 0, st, f0, f1, lin, hw, scratch); break;
  }
  hipLaunchKernelGGL(lpips_layer_final_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, scratch, n, bps, hw, accumulate, res);
  return check_launch("ldmk_lpips_layer");
}

extern "C" int ldmk_lpips_layer_bwd(const float* fa, const float* fb, const float* lin, const float* g, float* df, int relu_mask,
                                    int accumulate, int n, int hw, int c, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(fa && fb && lin && g && df && n > 0 && hw > 0, "ldmk_lpips_layer_bwd: bad args");
  LDMK_REQUIRE(lp_chan_ok(c), "ldmk_lpips_layer_bwd: C=%d is not one of 64, 128, 256, 512", c);
  LDMK_REQUIRE(lp_al16(fa) && lp_al16(fb) && lp_al16(lin) && lp_al16(df),
               "ldmk_lpips_layer_bwd: the taps, the weight and df must be 16-byte aligned");
  const long long pixels = (long long)n * hw;
  const dim3 grid(lp_grid(pixels, 4, LP_BLOCKS)), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (c) {
    case 64: hipLaunchKernelGGL(lpips_layer_bwd_kernel<1>, grid, block, 0, st, fa, fb, lin, g, df, hw, pixels, relu_mask, accumulate); break;
    case 128: hipLaunchKernelGGL(lpips_layer_bwd_kernel<2>, grid, block, 0, st, fa, fb, lin, g, df, hw, pixels, relu_mask, accumulate); break;
    case 256: hipLaunchKernelGGL(lpips_layer_bwd_kernel<4>, grid, block, 0, st, fa, fb, lin, g, df, hw, pixels, relu_mask, accumulate); break;
    default: hipLaunchKernelGGL(lpips_layer_bwd_kernel<8>, grid, block, 0, st, fa, fb, lin, g, df, hw, pixels, relu_mask, accumulate); break;
  }
  return check_launch("ldmk_lpips_layer_bwd");
}
