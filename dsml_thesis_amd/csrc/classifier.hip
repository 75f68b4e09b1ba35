// The pooled heads of EncoderUNetModel (openaimodel.py:751-961: adaptive, attention, spatial, spatial_v2) and the softmax
// cross-entropy of NoisyLatentImageClassifier (classifier.py:170-185).  gfx950 only.
// The conventions of objective.hip / kl_train.hip: fp32 in and out, no float atomics, every sum kept in double in one fixed order:
// bitwise reproducible.  The heads work on (n, hw <= a few thousand, C) activations and (n, K <= 1024) logits: a few launches of a
// few microseconds at the end of a step the torso dominates, so the kernels are written for exactness, not for occupancy.
#include "ldmk_common.h"
#include <math.h>

namespace ldmk {

constexpr int POOL_RG = 4;          // row groups of a 256-thread workgroup; 64 channel lanes each
constexpr int APOOL_MAX_T = 4096;   // tokens of the single-query attention: p and ds live in LDS (2 x 16 KB)
constexpr int APOOL_MAX_D = 128;

// Column sums over the hw rows of sample blockIdx.y for the 64 channels of blockIdx.x: row group g adds rows g, g + 4, ... in
// order, the four partials are added in group order.  Returns the sum in the threads of group 0 (others: unspecified).
__device__ __forceinline__ double pool_colsum(const float* __restrict__ xb, int hw, int c, int ch, int rg, double (*red)[64]) {
  double s = 0.0;
  if (ch < c)
    for (int i = rg; i < hw; i += POOL_RG) s += (double)xb[(long long)i * c + ch];
  red[rg][threadIdx.x & 63] = s;
  __syncthreads();
  return (red[0][threadIdx.x & 63] + red[1][threadIdx.x & 63]) + (red[2][threadIdx.x & 63] + red[3][threadIdx.x & 63]);
}

__global__ __launch_bounds__(256) void pool_mean_kernel(const float* __restrict__ x, float* __restrict__ feat, int hw, int c, int ld,
                                                        int col) {
  __shared__ double red[POOL_RG][64];
  const int b = blockIdx.y, ch = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
  const double s = pool_colsum(x + (long long)b * hw * c, hw, c, ch, rg, red);
  if (rg == 0 && ch < c) feat[(long long)b * ld + col + ch] = (float)(s / (double)hw);
}

__global__ __launch_bounds__(256) void pool_mean_bwd_kernel(const float* __restrict__ dfeat, float* __restrict__ dx, long long total,
                                                            int hw, int c, int ld, int col, int accumulate) {
  const float fhw = (float)hw;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ch = (int)(i % c);
    const long long b = i / ((long long)hw * c);
    const float g = dfeat[b * ld + col + ch] / fhw;
    dx[i] = accumulate ? dx[i] + g : g;
  }
}

__global__ __launch_bounds__(256) void attnpool_tokens_kernel(const float* __restrict__ y, const float* __restrict__ pos_t,
                                                              float* __restrict__ X, int hw, int c) {
  __shared__ double red[POOL_RG][64];
  const int b = blockIdx.y, ch = blockIdx.x * 64 + (threadIdx.x & 63), rg = threadIdx.x >> 6;
  const float* yb = y + (long long)b * hw * c;
  float* Xb = X + (long long)b * (hw + 1) * c;
  if (ch < c)
    for (int i = rg; i < hw; i += POOL_RG) Xb[(long long)(i + 1) * c + ch] = yb[(long long)i * c + ch] + pos_t[(long long)(i + 1) * c + ch];
  const double s = pool_colsum(yb, hw, c, ch, rg, red);
  if (rg == 0 && ch < c) Xb[ch] = (float)(s / (double)hw) + pos_t[ch];
}

// One thread per (token t, channel k): walks the samples in order.
__global__ __launch_bounds__(256) void attnpool_tokens_bwd_kernel(const float* __restrict__ dX, float* __restrict__ dy,
                                                                  float* __restrict__ dpos_t, int n, int hw, int c, int acc_dpos) {
  const long long per = (long long)(hw + 1) * c;
  const float fhw = (float)hw;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long long)gridDim.x * 256) {
    const int ch = (int)(i % c);
    const long long t = i / c;
    double s = 0.0;
    for (int b = 0; b < n; ++b) {
      const float v = dX[b * per + i];
      s += (double)v;
      if (dy && t > 0) dy[((long long)b * hw + (t - 1)) * c + ch] = v + dX[b * per + ch] / fhw;
    }
    if (dpos_t) dpos_t[i] = acc_dpos ? dpos_t[i] + (float)s : (float)s;
  }
}

// One wave per (sample, head).  Lanes over tokens for the logits, lanes over channels for the output.
__global__ __launch_bounds__(64) void attnpool_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                          float* __restrict__ probs, int T, int heads, int d, float scale) {
  __shared__ float q0[APOOL_MAX_D];
  __shared__ float p[APOOL_MAX_T];
  const int h = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int C3 = 3 * heads * d, C = heads * d;
  const float* base = qkv + (long long)b * T * C3;
  for (int k = lane; k < d; k += 64) q0[k] = base[h * d + k];
  __syncthreads();
  float mx = -INFINITY;
  for (int t = lane; t < T; t += 64) {
    const float4* kr = reinterpret_cast<const float4*>(base + (long long)t * C3 + C + h * d);
    double s = 0.0;
    for (int k4 = 0; k4 < d / 4; ++k4) {
      const float4 kv = kr[k4];
      s += (double)q0[4 * k4] * (double)kv.x + (double)q0[4 * k4 + 1] * (double)kv.y + (double)q0[4 * k4 + 2] * (double)kv.z +
           (double)q0[4 * k4 + 3] * (double)kv.w;
    }
    const float sf = (float)s * scale;
    p[t] = sf;
    mx = fmaxf(mx, sf);
  }
  mx = wave_max(mx);
  double z = 0.0;
  for (int t = lane; t < T; t += 64) {
    const float e = expf(p[t] - mx);
    p[t] = e;
    z += (double)e;
  }
  z = wave_sum_d(z);
  float* pr = probs + ((long long)b * heads + h) * T;
  for (int t = lane; t < T; t += 64) {
    const float v = (float)((double)p[t] / z);
    p[t] = v;
    pr[t] = v;
  }
  __syncthreads();
  for (int k = lane; k < d; k += 64) {
    const float* vc = base + 2 * C + h * d + k;
    double o = 0.0;
    for (int t = 0; t < T; ++t) o += (double)p[t] * (double)vc[(long long)t * C3];
    out[(long long)b * C + h * d + k] = (float)o;
  }
}

__global__ __launch_bounds__(64) void attnpool_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ probs,
                                                          const float* __restrict__ dout, float* __restrict__ dqkv, int T, int heads,
                                                          int d, float scale) {
  __shared__ float q0[APOOL_MAX_D], go[APOOL_MAX_D], dq0[APOOL_MAX_D];
  __shared__ float p[APOOL_MAX_T], ds[APOOL_MAX_T];
  const int h = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int C3 = 3 * heads * d, C = heads * d;
  const float* base = qkv + (long long)b * T * C3;
  float* dbase = dqkv + (long long)b * T * C3;
  const float* pr = probs + ((long long)b * heads + h) * T;
  for (int k = lane; k < d; k += 64) {
    q0[k] = base[h * d + k];
    go[k] = dout[(long long)b * C + h * d + k];
  }
  __syncthreads();
  double S = 0.0;                                  // sum_u p_u (dout . v_u)
  for (int t = lane; t < T; t += 64) {
    const float4* vr = reinterpret_cast<const float4*>(base + (long long)t * C3 + 2 * C + h * d);
    double g = 0.0;
    for (int k4 = 0; k4 < d / 4; ++k4) {
      const float4 vv = vr[k4];
      g += (double)go[4 * k4] * (double)vv.x + (double)go[4 * k4 + 1] * (double)vv.y + (double)go[4 * k4 + 2] * (double)vv.z +
           (double)go[4 * k4 + 3] * (double)vv.w;
    }
    const float pt = pr[t];
    p[t] = pt;
    ds[t] = (float)g;                              // dout . v_t for now
    S += (double)pt * g;
  }
  S = wave_sum_d(S);
  for (int t = lane; t < T; t += 64) ds[t] = (float)((double)p[t] * ((double)ds[t] - S));
  __syncthreads();
  for (int k = lane; k < d; k += 64) {
    const float* kc = base + C + h * d + k;
    double a = 0.0;
    for (int t = 0; t < T; ++t) a += (double)ds[t] * (double)kc[(long long)t * C3];
    dq0[k] = (float)(a * (double)scale);
  }
  __syncthreads();
  for (int i = lane; i < T * d; i += 64) {
    const int t = i / d, k = i - t * d;
    float* row = dbase + (long long)t * C3 + h * d + k;
    row[0] = t == 0 ? dq0[k] : 0.f;
    row[C] = scale * ds[t] * q0[k];
    row[2 * C] = p[t] * go[k];
  }
}

// One wave per sample.
__global__ __launch_bounds__(64) void cross_entropy_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                           float* __restrict__ per_sample, float* __restrict__ dlogits, float scale,
                                                           int K) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* lr = logits + (long long)b * K;
  long long y = target[b];
  y = y < 0 ? 0 : (y >= K ? K - 1 : y);
  float mx = -INFINITY;
  for (int k = lane; k < K; k += 64) mx = fmaxf(mx, lr[k]);
  mx = wave_max(mx);
  double z = 0.0;
  for (int k = lane; k < K; k += 64) z += exp((double)lr[k] - (double)mx);
  z = wave_sum_d(z);
  const double lse = log(z);                       // of the max-subtracted logits
  if (lane == 0) per_sample[b] = (float)(lse - ((double)lr[y] - (double)mx));
  if (dlogits)
    for (int k = lane; k < K; k += 64) {
      const double sm = exp(((double)lr[k] - (double)mx) - lse);
      dlogits[(long long)b * K + k] = (float)((sm - (k == y ? 1.0 : 0.0)) * (double)scale);
    }
}

__global__ __launch_bounds__(64) void cross_entropy_mean_kernel(const float* __restrict__ per_sample, float* __restrict__ mean, int n) {
  double s = 0.0;
  if (threadIdx.x == 0) {
    for (int b = 0; b < n; ++b) s += (double)per_sample[b];
    mean[0] = (float)(s / (double)n);
  }
}

__global__ __launch_bounds__(256) void relu_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) y[i] = fmaxf(x[i], 0.f);
}

__global__ __launch_bounds__(256) void relu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                                       long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dx[i] = x[i] > 0.f ? dy[i] : 0.f;
}

inline unsigned flat_grid(long long total) {
  const long long g = (total + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

}  // namespace ldmk

using namespace ldmk;

extern "C" int ldmk_pool_mean(const float* x, float* feat, int n, int hw, int c, int ld, int col, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(x && feat && n > 0 && hw > 0 && c > 0, "ldmk_pool_mean: bad args");
  LDMK_REQUIRE(col >= 0 && (long long)col + c <= ld, "ldmk_pool_mean: columns [%d, %d) outside a row of %d", col, col + c, ld);
  LDMK_REQUIRE(n <= 65535, "ldmk_pool_mean: n=%d above 65535 samples", n);
  hipLaunchKernelGGL(pool_mean_kernel, dim3((unsigned)((c + 63) / 64), (unsigned)n), dim3(256), 0, (hipStream_t)stream, x, feat, hw, c,
                     ld, col);
  return check_launch("ldmk_pool_mean");
}

extern "C" int ldmk_pool_mean_bwd(const float* dfeat, float* dx, int n, int hw, int c, int ld, int col, int accumulate, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(dfeat && dx && n > 0 && hw > 0 && c > 0, "ldmk_pool_mean_bwd: bad args");
  LDMK_REQUIRE(col >= 0 && (long long)col + c <= ld, "ldmk_pool_mean_bwd: columns [%d, %d) outside a row of %d", col, col + c, ld);
  const long long total = (long long)n * hw * c;
  hipLaunchKernelGGL(pool_mean_bwd_kernel, dim3(flat_grid(total)), dim3(256), 0, (hipStream_t)stream, dfeat, dx, total, hw, c, ld, col,
                     accumulate);
  return check_launch("ldmk_pool_mean_bwd");
}

extern "C" int ldmk_attnpool_tokens(const float* y, const float* pos_t, float* X, int n, int hw, int c, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(y && pos_t && X && n > 0 && hw > 0 && c > 0, "ldmk_attnpool_tokens: bad args");
  LDMK_REQUIRE(n <= 65535, "ldmk_attnpool_tokens: n=%d above 65535 samples", n);
  hipLaunchKernelGGL(attnpool_tokens_kernel, dim3((unsigned)((c + 63) / 64), (unsigned)n), dim3(256), 0, (hipStream_t)stream, y, pos_t,
                     X, hw, c);
  return check_launch("ldmk_attnpool_tokens");
}

extern "C" int ldmk_attnpool_tokens_bwd(const float* dX, float* dy, float* dpos_t, int n, int hw, int c, int acc_dpos, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(dX && (dy || dpos_t) && n > 0 && hw > 0 && c > 0, "ldmk_attnpool_tokens_bwd: bad args");
  hipLaunchKernelGGL(attnpool_tokens_bwd_kernel, dim3(flat_grid((long long)(hw + 1) * c)), dim3(256), 0, (hipStream_t)stream, dX, dy,
                     dpos_t, n, hw, c, acc_dpos);
  return check_launch("ldmk_attnpool_tokens_bwd");
}

static int attnpool_check(const char* who, const void* qkv, int n, int T, int heads, int d_head) {
  LDMK_REQUIRE(n > 0 && T > 0 && heads > 0, "%s: n, T and heads must be positive", who);
  LDMK_REQUIRE(d_head >= 4 && d_head <= APOOL_MAX_D && d_head % 4 == 0, "%s: d_head=%d (a multiple of 4 in [4, %d])", who, d_head,
               APOOL_MAX_D);
  LDMK_REQUIRE(T <= APOOL_MAX_T, "%s: T=%d tokens above %d", who, T, APOOL_MAX_T);
  LDMK_REQUIRE(n <= 65535, "%s: n=%d above 65535 samples", who, n);
  LDMK_REQUIRE(((uintptr_t)qkv & 15) == 0, "%s: qkv off a 16-byte boundary", who);
  return LDMK_OK;
}

extern "C" int ldmk_attnpool_fwd(const float* qkv, float* out, float* probs, int n, int T, int heads, int d_head, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(qkv && out && probs, "ldmk_attnpool_fwd: bad args");
  if (int rc = attnpool_check("ldmk_attnpool_fwd", qkv, n, T, heads, d_head)) return rc;
  hipLaunchKernelGGL(attnpool_fwd_kernel, dim3((unsigned)heads, (unsigned)n), dim3(64), 0, (hipStream_t)stream, qkv, out, probs, T,
                     heads, d_head, 1.0f / sqrtf((float)d_head));
  return check_launch("ldmk_attnpool_fwd");
}

extern "C" int ldmk_attnpool_bwd(const float* qkv, const float* probs, const float* dout, float* dqkv, int n, int T, int heads,
                                 int d_head, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(qkv && probs && dout && dqkv, "ldmk_attnpool_bwd: bad args");
  if (int rc = attnpool_check("ldmk_attnpool_bwd", qkv, n, T, heads, d_head)) return rc;
  hipLaunchKernelGGL(attnpool_bwd_kernel, dim3((unsigned)heads, (unsigned)n), dim3(64), 0, (hipStream_t)stream, qkv, probs, dout, dqkv,
                     T, heads, d_head, 1.0f / sqrtf((float)d_head));
  return check_launch("ldmk_attnpool_bwd");
}

extern "C" int ldmk_cross_entropy(const float* logits, const long long* target, float* per_sample, float* mean, float* dlogits,
                                  float scale, int n, int K, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(logits && target && per_sample && mean && n > 0, "ldmk_cross_entropy: bad args");
  LDMK_REQUIRE(K >= 1 && K <= 1024, "ldmk_cross_entropy: K=%d classes outside [1, 1024]", K);
  hipLaunchKernelGGL(cross_entropy_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, logits, target, per_sample, dlogits,
                     scale, K);
  hipLaunchKernelGGL(cross_entropy_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, per_sample, mean, n);
  return check_launch("ldmk_cross_entropy");
}

extern "C" int ldmk_relu(const float* x, float* y, long long n, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(x && y && n > 0, "ldmk_relu: bad args");
  hipLaunchKernelGGL(relu_kernel, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, x, y, n);
  return check_launch("ldmk_relu");
}

extern "C" int ldmk_relu_bwd(const float* x, const float* dy, float* dx, long long n, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(x && dy && dx && n > 0, "ldmk_relu_bwd: bad args");
  hipLaunchKernelGGL(relu_bwd_kernel, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, n);
  return check_launch("ldmk_relu_bwd");
}
