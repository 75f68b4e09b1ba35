// The lane = column epilogue of the implicit GEMMs: igemm_ws_kernel (igemm_ws.hip) and the non-transposed ps_epilogue
// (igemm_ps.hip) finish a wave's acc[TM][TN] 32x32 tiles at (rowbase, colbase) with the pieces below.  igemm_kernel (igemm.hip)
// keeps a copy of its own (see its epilogue for why) and shares the finishers.
// C/D map of the 32x32 MFMA: col = lane & 31 (l31), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (half).
// The order of the roundings is a contract: the pre-split and warp-specialised tiles promise the bits of tile_cfg 1 / 5
// (tests/test_ps_gpu.py, tests/test_split_gpu.py, tests/test_ps_conv_gpu.py), and the lean forms promise the bits of the general
// one.  The transposed epilogue of igemm_ps.hip, rgemm.hip and sgemm.hip (lane = row maps) use the scalar helpers and the
// GroupNorm record from here and keep their own bodies.
#pragma once
#include "ldmk_common.h"

namespace ldmk {

// the folded LayerNorm of one accumulator value + bias: rstd (acc - mean colsum) + b with the roundings of the general form below
// and of rgemm.hip -- one fma, one multiply, one add.  Contraction is switched off here: in the general epilogue a select sits
// between the multiply and the add, in a lean one nothing does, and the compiler would fuse them into a second fma (one rounding
// less: other bits).
__device__ __forceinline__ float lnf_bias(float acc, float mean, float cs, float rstd, float bias) {
#pragma clang fp contract(off)
  const float t = __builtin_fmaf(-mean, cs, acc) * rstd;
  return t + bias;
}
// the same for a launch without a folded LayerNorm: alpha acc + b (+ 0 for the absent per-sample vector) + residual, each its own
// rounding as in the general epilogue (where the `if (lnf)` select sits between the multiply and the first add)
__device__ __forceinline__ float bias_res(float acc_alpha, float bias, float vec, float res) {
#pragma clang fp contract(off)
  float t = acc_alpha + bias;
  t = t + vec;                 // (the per-sample vector, or +0 where the general form adds its zero)
  return t + res;
}
// lane = column form: alpha acc + bias [+ per-sample vector | + residual], each addition its own rounding as in the general form
__device__ __forceinline__ float col_finish(float acc_alpha, float bias) {
#pragma clang fp contract(off)
  return acc_alpha + bias;
}
__device__ __forceinline__ float col_finish(float acc_alpha, float bias, float extra) {
#pragma clang fp contract(off)
  const float t = acc_alpha + bias;
  return t + extra;
}
__device__ __forceinline__ float col_finish(float acc_alpha, float bias, float vec, float res) {
#pragma clang fp contract(off)
  float t = acc_alpha + bias;
  t = t + vec;
  return t + res;
}

// GroupNorm partial record of one 32-row tile x column (same record as gn_partial_kernel): the 32 rows of the tile sit in
// 16 registers x 2 half-waves of the lane pair (l31, l31 + 32); three floats per tile and column: shift, sum (x - shift),
// sum (x - shift)^2, shift = the fp32 mean of the tile's 32 values.  The caller guards (stats_out set, tile inside M).
__device__ __forceinline__ void gn_tile_record(const float (&vals)[16], float* stats_out, const int tile_row, const int N,
                                               const int col, const int l31, const int half) {
  // shift = the tile's own mean (any fp32 value serves: the finalize un-shifts in double with the stored one).  With row 0 as the
  // shift an outlier first row left partial sums of ~70 sigma-units and 2-6 x 2^-24 of error in the group mean.
  float tsum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) tsum += vals[r];
  tsum += __shfl_xor(tsum, 32, 64);                   // (a + b == b + a: both halves hold the same bits)
  const float shift = tsum * (1.0f / 32.0f);
  float sm = 0.f, sq = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float d = vals[r] - shift;
    sm += d;
    sq = fmaf(d, d, sq);
  }
  sm += __shfl_xor(sm, 32, 64);
  sq += __shfl_xor(sq, 32, 64);
  if (half == 0) {
    float* d = stats_out + ((long long)tile_row * N + col) * 3;
    d[0] = shift; d[1] = sm; d[2] = sq;
  }
}

// The same record with the three sums taken over the tile's 32 rows ONE AFTER THE OTHER, rows 0..31 -- the order of
// igemm_reduce_stats_kernel (igemm.hip), which writes the records of a launch split over workgroups.  The K groups inside the
// workgroup (igemm_ps.hip, KG = 2) promise the bits of that two-launch form, records included, so that a shape may move between
// the two without its GroupNorm changing.  Rows 8 g + 4 half + e sit at vals[4 g + e]: the running sum crosses between the half-
// waves eight times, each crossing one v_permlane32_swap (both halves then hold the sending half's value).
__device__ __forceinline__ float gn_other_half(float x, const bool from_upper) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(from_upper ? r[1] : r[0]);
}
__device__ __forceinline__ void gn_tile_record_rows(const float (&vals)[16], float* stats_out, const int tile_row, const int N,
                                                    const int col, const int l31, const int half) {
#pragma clang fp contract(off)
  float tsum = 0.f;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int e = 0; e < 4; ++e) tsum += vals[4 * g + e];           // (meaningful in the lower half)
    tsum = gn_other_half(tsum, false);
#pragma unroll
    for (int e = 0; e < 4; ++e) tsum += vals[4 * g + e];           // (meaningful in the upper half)
    tsum = gn_other_half(tsum, true);
  }
  const float shift = tsum * (1.0f / 32.0f);
  float sm = 0.f, sq = 0.f;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = vals[4 * g + e] - shift;
      sm += d;
      sq = fmaf(d, d, sq);
    }
    sm = gn_other_half(sm, false);
    sq = gn_other_half(sq, false);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = vals[4 * g + e] - shift;
      sm += d;
      sq = fmaf(d, d, sq);
    }
    sm = gn_other_half(sm, true);
    sq = gn_other_half(sq, true);
  }
  if (half == 0) {
    float* d = stats_out + ((long long)tile_row * N + col) * 3;
    d[0] = shift; d[1] = sm; d[2] = sq;
  }
}

// split-K: the raw partial slab [ks][M][N]; igemm_reduce_kernel or the consumer (raw_slabs) sums them
template <int TM, int TN>
__device__ __forceinline__ void col_slab_store(const ldmk_igemm_args& p, const f32x16 (&acc)[TM][TN], const int rowbase, const int colbase,
                                               const int bz, const int l31, const int half, const int splitk, const int ks,
                                               float* __restrict__ ws) {
  float* slab = ws + ((long long)bz * splitk + ks) * p.M * p.N;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = colbase + j * 32 + l31;
    if (col >= p.N) continue;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = rowbase + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row < p.M) slab[(long long)row * p.N + col] = acc[i][j][r];
      }
  }
}

// GEGLU: tile j holds the packed value columns, tile j + 1 their gates; out = (v + b_v) gelu(g + b_g), N / 2 output columns.
// lnf: the LayerNorm folded through the product (two per-row scalars here) -- same arithmetic as rgemm.hip and igemm_reduce_kernel.
template <int TM, int TN>
__device__ __forceinline__ void col_geglu(const ldmk_igemm_args& p, const f32x16 (&acc)[TM][TN], const int rowbase, const int colbase,
                                          const int bz, const int l31, const int half, const bool lnf) {
  float* __restrict__ outp = p.out + (long long)bz * p.out_bstride;
  const float alpha = p.alpha;
  const float2* __restrict__ stats2 = reinterpret_cast<const float2*>(p.row_stats);
  if constexpr (TN % 2 == 0) {
#pragma unroll
    for (int j = 0; j < TN; j += 2) {
      const int cv = colbase + j * 32 + l31;        // packed value column
      const int cg = cv + 32;                       // packed gate column
      if (cv >= p.N) continue;
      const int oc = ((colbase + j * 32) >> 1) + l31;
      const float bv = p.bias ? p.bias[cv] : 0.f, bg = p.bias ? p.bias[cg] : 0.f;
      const float csv = lnf ? p.ln_colsum[cv] : 0.f, csg = lnf ? p.ln_colsum[cg] : 0.f;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        float2 st[16];
        if (lnf) {
#pragma unroll
          for (int r = 0; r < 16; ++r) st[r] = stats2[min(rowbase + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, p.M - 1)];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = rowbase + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          if (row < p.M) {
            float v = acc[i][j][r] * alpha, g = acc[i][j + 1][r] * alpha;
            if (lnf) {
              v = fmaf(-st[r].x, csv, v) * st[r].y;
              g = fmaf(-st[r].x, csg, g) * st[r].y;
            }
            v += bv;
            g += bg;
            const float ge = gelu_erf_f(g);                                            // exact (erf) GELU
            outp[(long long)row * p.ldc + oc] = v * ge;
          }
        }
      }
    }
  }
}

// The general form: [folded LayerNorm] -> bias -> per-sample vector -> residual, every element behind its row predicate, then
// the GroupNorm record.  Element offsets are 32-bit (the host checks M * ldc < 2^31): one add per address; the per-sample vector
// is looked up once per 32-row tile when a tile cannot straddle two samples (rows_per_sample % 32 == 0: every UNet / VQGAN
// level) instead of one integer division per output element.  (acc is scratch here: the folded LayerNorm rewrites it.)
template <int TM, int TN, bool ROWREC = false>      // ROWREC: the record in row order (gn_tile_record_rows)
__device__ __forceinline__ void col_general(const ldmk_igemm_args& p, f32x16 (&acc)[TM][TN], const int rowbase, const int colbase,
                                            const int bz, const int l31, const int half, const bool lnf) {
  float* __restrict__ outp = p.out + (long long)bz * p.out_bstride;
  const float* resp = p.residual ? p.residual + (long long)bz * p.out_bstride : nullptr;
  const float alpha = p.alpha;
  const float2* __restrict__ stats2 = reinterpret_cast<const float2*>(p.row_stats);
  const bool tile_in_sample = p.rows_per_sample % 32 == 0;
  int smp[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) smp[i] = p.batch_vec ? min(rowbase + i * 32, p.M - 1) / p.rows_per_sample : 0;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = colbase + j * 32 + l31;
    if (col >= p.N) continue;
    const float bv = p.bias ? p.bias[col] : 0.f;
    const float cs = lnf ? p.ln_colsum[col] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      float vals[16];
      const int r0 = rowbase + i * 32 + 4 * half;
      if (lnf) {
        float2 st[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = stats2[min(r0 + (r & 3) + 8 * (r >> 2), p.M - 1)];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = fmaf(-st[r].x, cs, acc[i][j][r] * alpha) * st[r].y;
      }
      const unsigned obase = (unsigned)r0 * (unsigned)p.ldc + (unsigned)col;
      const float vec = (p.batch_vec && tile_in_sample) ? p.batch_vec[(long long)smp[i] * p.batch_vec_ld + col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int dr = (r & 3) + 8 * (r >> 2);
        float v = 0.f;
        if (r0 + dr < p.M) {
          v = (lnf ? acc[i][j][r] : acc[i][j][r] * alpha) + bv;
          if (p.batch_vec) v += tile_in_sample ? vec : p.batch_vec[(long long)((r0 + dr) / p.rows_per_sample) * p.batch_vec_ld + col];
          const unsigned o = obase + (unsigned)(dr * p.ldc);
          if (resp) v += resp[o];
          outp[o] = v;
        }
        vals[r] = v;
      }
      if (p.stats_out && rowbase + i * 32 < p.M) {
        if constexpr (ROWREC) gn_tile_record_rows(vals, p.stats_out, (rowbase + i * 32) >> 5, p.N, col, l31, half);
        else gn_tile_record(vals, p.stats_out, (rowbase + i * 32) >> 5, p.N, col, l31, half);
      }
    }
  }
}

// The lean form (one wave tile wholly inside M x N, no split-K, no folded LayerNorm, no GEGLU, 32-row tiles inside one sample:
// col_lean_form below): no per-element row predicate and operand branches -- in the general form every residual load sits in its
// own basic block and waits for itself (577 s_waitcnt in the 160 -> 160 convolution's kernel); here the 16 residuals of a tile
// are asked for at once -- and the operand set is a template argument: 1 = per-sample vector, 2 = residual, 3 = neither,
// 4 = both.  Same arithmetic, rounding by rounding, as the general form.
template <int TM, int TN, int LEAN, bool ROWREC = false>
__device__ __forceinline__ void col_lean(const ldmk_igemm_args& p, const f32x16 (&acc)[TM][TN], const int rowbase, const int colbase,
                                         const int bz, const int l31, const int half) {
  static_assert(LEAN >= 1 && LEAN <= 4, "operand set 1..4");
  float* __restrict__ outp = p.out + (long long)bz * p.out_bstride;
  const float* __restrict__ resp = (LEAN == 2 || LEAN == 4) ? p.residual + (long long)bz * p.out_bstride : nullptr;
  const float alpha = p.alpha;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = colbase + j * 32 + l31;
    const float bv = p.bias ? p.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int r0 = rowbase + i * 32 + 4 * half;
      const unsigned obase = (unsigned)r0 * (unsigned)p.ldc + (unsigned)col;
      float extra[16], vec = 0.f;
      if constexpr (LEAN == 1 || LEAN == 4) vec = p.batch_vec[(long long)((rowbase + i * 32) / p.rows_per_sample) * p.batch_vec_ld + col];
      if constexpr (LEAN == 2 || LEAN == 4) {
#pragma unroll
        for (int r = 0; r < 16; ++r) extra[r] = resp[obase + (unsigned)(((r & 3) + 8 * (r >> 2)) * p.ldc)];
      }
      float vals[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float t = acc[i][j][r] * alpha;
        if constexpr (LEAN == 3) vals[r] = col_finish(t, bv);
        else if constexpr (LEAN == 1) vals[r] = col_finish(t, bv, vec);
        else if constexpr (LEAN == 2) vals[r] = col_finish(t, bv, extra[r]);
        else vals[r] = col_finish(t, bv, vec, extra[r]);
        outp[obase + (unsigned)(((r & 3) + 8 * (r >> 2)) * p.ldc)] = vals[r];
      }
      if (p.stats_out) {
        if constexpr (ROWREC) gn_tile_record_rows(vals, p.stats_out, (rowbase + i * 32) >> 5, p.N, col, l31, half);
        else gn_tile_record(vals, p.stats_out, (rowbase + i * 32) >> 5, p.N, col, l31, half);
      }
    }
  }
}

// THE predicate: which lean form (col_lean's LEAN) a wave tile ending at (row_end, col_end) may take; 0 = the general one.
// Wave-uniform.  off: the launch asked for the general form everywhere (A/B switch LDMK_PS_LEAN=0).
__device__ __forceinline__ int col_lean_form(const ldmk_igemm_args& p, const int splitk, const bool off, const int row_end, const int col_end) {
  if (off || splitk != 1 || row_end > p.M || col_end > p.N) return 0;
  if (p.batch_vec && p.rows_per_sample % 32 != 0) return 0;      // (a 32-row tile inside one sample)
  if (p.a_tf == LDMK_TF_LAYERNORM_FOLDED || p.epi == LDMK_EPI_GEGLU) return 0;
  return p.batch_vec ? (p.residual ? 4 : 1) : (p.residual ? 2 : 3);
}

}  // namespace ldmk
