// The update kernels under `DPM_Solver.sample` (dpm_solver.py:386-399, 504-857) beyond ldmk_dpm_step (small.hip): one stage-structured
// update per model evaluation for the singlestep and multistep solvers in both forms and both solver types, the unthresholded data
// prediction, and the per-sample quantile of dynamic thresholding.  gfx950 only.  fp32, every operation rounded on its own
// (no contraction) in the reference's order; no float atomics: bitwise reproducible.
#include "ldmk_common.h"
#include <math.h>

namespace ldmk {

// One row of STG_ROW floats per model evaluation (include/ldmk.h, ldmk_dpm_stage, has the layout).
enum { STG_ROW = 16, STG_NEXT_T = 15, STG_FLAGS = 14 };
enum { STG_SS_FIRST = 0, STG_SS_MID = 1, STG_SS_LAST = 2, STG_SS_TAYLOR3 = 3, STG_MS1 = 4, STG_MS2 = 5, STG_MS3 = 6, STG_DENOISE = 7 };
enum { STG_F_X0 = 1, STG_F_THRESHOLD = 2 };
enum { STG_USES_KEEP = 1, STG_USES_RING = 2 };

__device__ __forceinline__ int stg_row_index(const int* step_idx, int n_rows) {
  int k = *step_idx;                                 // (a captured step replayed past the end stays on the last row)
  if (k > n_rows - 1) k = n_rows - 1;
  return k < 0 ? 0 : k;
}

__device__ __forceinline__ float stg_eps(const float* __restrict__ eps, long long i, long long total, float cfg_scale, int cfg) {
  if (!cfg) return eps[i];
  const float eu = eps[i], ec = eps[total + i];
  return __fadd_rn(eu, __fmul_rn(cfg_scale, __fsub_rn(ec, eu)));
}

// (x_prev may be x, so neither is __restrict__; keep and hist are only touched by the kinds that name them)
__global__ void dpm_stage_kernel(const float* x, const float* __restrict__ eps, const float* __restrict__ table,
                                 const int* __restrict__ step_idx, int n_rows, float cfg_scale, int cfg,
                                 const float* __restrict__ x0_pre, const float* __restrict__ s, float* __restrict__ keep,
                                 float* __restrict__ hist, float* x_prev, float* __restrict__ model_out, long long per,
                                 long long total, int uses) {
  const int k = stg_row_index(step_idx, n_rows);
  const float* __restrict__ row = table + (long long)STG_ROW * k;
  const float alpha = row[0], sigma = row[1], c_x = row[3], c_0 = row[4], p5 = row[5], p6 = row[6], p7 = row[7], p8 = row[8],
              c_1 = row[9], c_2 = row[10], p11 = row[11];
  const int kind = (int)row[2], flags = (int)row[STG_FLAGS];
  const bool x0_form = flags & STG_F_X0, thresholded = (flags & STG_F_THRESHOLD) && x0_pre && s;
  const bool on_keep = kind >= STG_SS_FIRST && kind <= STG_SS_TAYLOR3, on_ring = kind >= STG_MS1 && kind <= STG_MS3;
  const bool allowed = (on_keep && (uses & STG_USES_KEEP) && keep) || (on_ring && (uses & STG_USES_RING) && hist) || kind == STG_DENOISE;
  float* __restrict__ keep_x = keep;
  float* __restrict__ keep_m = keep + total;
  float* __restrict__ keep_m1 = keep + 2 * total;
  float* __restrict__ h0 = hist + (long long)(k % 3) * total;
  const float* __restrict__ h1 = hist + (long long)((k + 2) % 3) * total;
  const float* __restrict__ h2 = hist + (long long)((k + 1) % 3) * total;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    if (!allowed) {                                  // a table this launch was not set up for: loud, and inside x' only
      x_prev[i] = __int_as_float(0x7fc00000);
      continue;
    }
    const float e = stg_eps(eps, i, total, cfg_scale, cfg);
    const float xv = x[i];
    float m;
    if (!x0_form) {
      m = e;
    } else if (thresholded) {
      const float sv = s[i / per], v = x0_pre[i];
      m = __fdiv_rn(v < -sv ? -sv : (v > sv ? sv : v), sv);          // (a NaN passes through, as torch.clamp)
    } else {
      m = __fdiv_rn(__fsub_rn(xv, __fmul_rn(sigma, e)), alpha);
    }
    float xt;
    switch (kind) {
      case STG_SS_FIRST:
        xt = __fsub_rn(__fmul_rn(c_x, xv), __fmul_rn(c_0, m));
        keep_x[i] = xv;
        keep_m[i] = m;
        break;
      case STG_SS_MID:
      case STG_SS_LAST: {
        const float ms = keep_m[i];
        xt = __fadd_rn(__fsub_rn(__fmul_rn(c_x, keep_x[i]), __fmul_rn(c_0, ms)), __fmul_rn(p5, __fsub_rn(m, ms)));
        if (kind == STG_SS_MID) keep_m1[i] = m;
        break;
      }
      case STG_SS_TAYLOR3: {
        const float ms = keep_m[i];
        const float d10 = __fmul_rn(p5, __fsub_rn(keep_m1[i], ms));
        const float d11 = __fmul_rn(p6, __fsub_rn(m, ms));
        const float d1 = __fdiv_rn(__fsub_rn(__fmul_rn(p8, d10), __fmul_rn(p7, d11)), p11);
        const float d2 = __fdiv_rn(__fmul_rn(2.f, __fsub_rn(d11, d10)), p11);
        xt = __fsub_rn(__fmul_rn(c_x, keep_x[i]), __fmul_rn(c_0, ms));
        xt = __fsub_rn(__fadd_rn(xt, __fmul_rn(c_1, d1)), __fmul_rn(c_2, d2));
        break;
      }
      case STG_MS1:
        xt = __fsub_rn(__fmul_rn(c_x, xv), __fmul_rn(c_0, m));
        h0[i] = m;
        break;
      case STG_MS2: {
        const float d10 = __fmul_rn(p5, __fsub_rn(m, h1[i]));
        xt = __fadd_rn(__fsub_rn(__fmul_rn(c_x, xv), __fmul_rn(c_0, m)), __fmul_rn(c_1, d10));
        h0[i] = m;
        break;
      }
      case STG_MS3: {
        const float m1 = h1[i];
        const float d10 = __fmul_rn(p5, __fsub_rn(m, m1));
        const float d11 = __fmul_rn(p6, __fsub_rn(m1, h2[i]));
        const float dd = __fsub_rn(d10, d11);
        const float d1 = __fadd_rn(d10, __fmul_rn(p7, dd));
        const float d2 = __fmul_rn(p8, dd);
        xt = __fsub_rn(__fmul_rn(c_x, xv), __fmul_rn(c_0, m));
        xt = __fsub_rn(__fadd_rn(xt, __fmul_rn(c_1, d1)), __fmul_rn(c_2, d2));
        h0[i] = m;
        break;
      }
      default:                                       // STG_DENOISE
        xt = m;
        break;
    }
    x_prev[i] = xt;
    if (model_out) model_out[i] = m;
  }
}

// runs after dpm_stage_kernel on the same stream: ts[0..n_ts) = the model time of the next row, step_idx one up
__global__ void dpm_stage_advance_kernel(int* step_idx, const float* __restrict__ table, float* __restrict__ ts, int n_ts, int n_rows) {
  const int k = stg_row_index(step_idx, n_rows);
  const float t = table[(long long)STG_ROW * k + STG_NEXT_T];
  for (int i = threadIdx.x; i < n_ts; i += blockDim.x) ts[i] = t;
  __syncthreads();
  if (threadIdx.x == 0) *step_idx = k + 1;
}

__global__ void dpm_predict_x0_kernel(const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ table,
                                      const int* __restrict__ step_idx, int n_rows, float cfg_scale, int cfg, float* __restrict__ x0,
                                      long long total) {
  const int k = stg_row_index(step_idx, n_rows);
  const float alpha = table[(long long)STG_ROW * k], sigma = table[(long long)STG_ROW * k + 1];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
    x0[i] = __fdiv_rn(__fsub_rn(x[i], __fmul_rn(sigma, stg_eps(eps, i, total, cfg_scale, cfg))), alpha);
}

// ---------------------------------------------------------------------------------------------
// s[r] = max(quantile(|v[r]|, q), floor_val).  One workgroup per row.  The keys are the bit patterns of |v| (sign bit cleared): for
// everything that is not a NaN their unsigned order is the order of the values, and every NaN sorts above +inf.  Four passes of an
// 8-bit radix select find the key of rank lo exactly: each pass counts, in an integer LDS histogram, the next digit of the keys that
// share the digits found so far, an exclusive scan of the 256 counts names the digit that holds the rank.  The last pass also tells
// how many keys are <= the one found; when rank hi lies beyond them its statistic is the smallest larger key (one more pass, an
// integer minimum).  Only integer atomics on LDS, whose result does not depend on their order.
constexpr int QT = 1024;
constexpr int QUANTILE_MAX_PER = 1 << 20;

__global__ __launch_bounds__(QT) void abs_quantile_rows_kernel(const float* __restrict__ v, int per, float q, float floor_val,
                                                               float* __restrict__ s_out) {
  __shared__ unsigned hist[256];
  __shared__ unsigned scan[2][256];
  __shared__ unsigned sh_digit, sh_rank, sh_eq, sh_min, sh_nan;
  const float* __restrict__ row = v + (long long)blockIdx.x * per;
  const int tid = threadIdx.x;
  const float rank = __fmul_rn(q, (float)(per - 1));
  const float lo = floorf(rank), hi = ceilf(rank), w = __fsub_rn(rank, lo);
  int ilo = (int)lo, ihi = (int)hi;
  ilo = ilo < 0 ? 0 : (ilo > per - 1 ? per - 1 : ilo);
  ihi = ihi < ilo ? ilo : (ihi > per - 1 ? per - 1 : ihi);
  if (tid == 0) {
    sh_nan = 0u;
    sh_min = 0xffffffffu;
  }
  unsigned prefix = 0u, mask = 0u, r = (unsigned)ilo, eq = 0u;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    for (int i = tid; i < per; i += QT) {
      const unsigned key = __float_as_uint(row[i]) & 0x7fffffffu;
      if (shift == 24 && key > 0x7f800000u) sh_nan = 1u;            // (every writer writes the same word)
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    // inclusive scan of the 256 counts (Hillis-Steele, ping-pong), by the first 256 threads
    if (tid < 256) scan[0][tid] = hist[tid];
    __syncthreads();
    int src = 0;
    for (int off = 1; off < 256; off <<= 1) {
      if (tid < 256) scan[src ^ 1][tid] = scan[src][tid] + (tid >= off ? scan[src][tid - off] : 0u);
      __syncthreads();
      src ^= 1;
    }
    if (tid < 256) {
      const unsigned incl = scan[src][tid], cnt = hist[tid], excl = incl - cnt;
      if (cnt > 0u && excl <= r && r < incl) {                       // exactly one digit holds rank r
        sh_digit = (unsigned)tid;
        sh_rank = r - excl;
        sh_eq = cnt;
      }
    }
    __syncthreads();
    prefix |= sh_digit << shift;
    mask |= 255u << shift;
    r = sh_rank;
    eq = sh_eq;
    __syncthreads();
  }
  const unsigned key_a = prefix;
  const unsigned n_le = ((unsigned)ilo - r) + eq;                    // keys <= key_a
  unsigned key_b = key_a;
  if ((unsigned)ihi >= n_le) {                                       // (uniform over the workgroup)
    for (int i = tid; i < per; i += QT) {
      const unsigned key = __float_as_uint(row[i]) & 0x7fffffffu;
      if (key > key_a) atomicMin(&sh_min, key);
    }
    __syncthreads();
    key_b = sh_min;
  }
  if (tid == 0) {
    const float a = __uint_as_float(key_a), b = __uint_as_float(key_b);
    const float d = __fsub_rn(b, a);
    float res = w < 0.5f ? __fmaf_rn(w, d, a) : __fmaf_rn(-d, __fsub_rn(1.f, w), b);     // torch's lerp: one fused rounding per branch
    if (sh_nan) res = __int_as_float(0x7fc00000);
    s_out[blockIdx.x] = (res != res) ? res : fmaxf(res, floor_val);  // (torch.maximum hands a NaN on)
  }
}

static inline int stage_grid(long long n) {
  long long b = (n + 255) / 256;
  return (int)(b > 4096 ? 4096 : b);
}

}  // namespace ldmk

using namespace ldmk;

extern "C" int ldmk_dpm_stage(const float* x, const float* eps, const float* table, int* step_idx, float cfg_scale, int cfg,
                              const float* x0_pre, const float* s, float* keep, float* hist, float* x_prev, float* model_out,
                              long long per_sample, int n, float* ts, int n_ts, int advance, int n_rows, int uses, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(x && eps && table && step_idx && x_prev, "ldmk_dpm_stage: null pointer (x, eps, table, step_idx, x_prev)");
  LDMK_REQUIRE(per_sample > 0 && n > 0 && n_rows > 0, "ldmk_dpm_stage: per_sample, n and n_rows must be positive");
  LDMK_REQUIRE(uses >= 1 && uses <= 3, "ldmk_dpm_stage: uses %d: bit 0 = singlestep rows (keep), bit 1 = multistep rows (hist)", uses);
  LDMK_REQUIRE(!(uses & STG_USES_KEEP) || keep, "ldmk_dpm_stage: singlestep rows need keep [3][n * per_sample]");
  LDMK_REQUIRE(!(uses & STG_USES_RING) || hist, "ldmk_dpm_stage: multistep rows need hist [3][n * per_sample]");
  LDMK_REQUIRE(!x0_pre == !s, "ldmk_dpm_stage: thresholding needs both x0_pre and s");
  if (advance) LDMK_REQUIRE(ts && n_ts > 0 && advance == 1, "ldmk_dpm_stage: advance (1: one row on) needs ts/n_ts");
  const long long total = per_sample * n;
  hipLaunchKernelGGL(dpm_stage_kernel, dim3(stage_grid(total)), dim3(256), 0, (hipStream_t)stream, x, eps, table, step_idx, n_rows,
                     cfg_scale, cfg, x0_pre, s, keep, hist, x_prev, model_out, per_sample, total, uses);
  if (advance)
    hipLaunchKernelGGL(dpm_stage_advance_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, step_idx, table, ts, n_ts, n_rows);
  return check_launch("ldmk_dpm_stage");
}

extern "C" int ldmk_dpm_predict_x0(const float* x, const float* eps, const float* table, const int* step_idx, float cfg_scale, int cfg,
                                   float* x0, long long per_sample, int n, int n_rows, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(x && eps && table && step_idx && x0, "ldmk_dpm_predict_x0: null pointer (x, eps, table, step_idx, x0)");
  LDMK_REQUIRE(per_sample > 0 && n > 0 && n_rows > 0, "ldmk_dpm_predict_x0: per_sample, n and n_rows must be positive");
  const long long total = per_sample * n;
  hipLaunchKernelGGL(dpm_predict_x0_kernel, dim3(stage_grid(total)), dim3(256), 0, (hipStream_t)stream, x, eps, table, step_idx, n_rows,
                     cfg_scale, cfg, x0, total);
  return check_launch("ldmk_dpm_predict_x0");
}

extern "C" int ldmk_abs_quantile_rows(const float* v, int rows, long long per, float q, float floor_val, float* s_out, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(v && s_out, "ldmk_abs_quantile_rows: null pointer (v, s_out)");
  LDMK_REQUIRE(rows > 0 && per > 0, "ldmk_abs_quantile_rows: rows and per must be positive");
  LDMK_REQUIRE(per <= QUANTILE_MAX_PER, "ldmk_abs_quantile_rows: per %lld: a row holds at most 2^20 = %d values", per, QUANTILE_MAX_PER);
  LDMK_REQUIRE(q >= 0.f && q <= 1.f, "ldmk_abs_quantile_rows: q %g is outside [0, 1]", (double)q);
  hipLaunchKernelGGL(abs_quantile_rows_kernel, dim3(rows), dim3(QT), 0, (hipStream_t)stream, v, (int)per, q, floor_val, s_out);
  return check_launch("ldmk_abs_quantile_rows");
}
