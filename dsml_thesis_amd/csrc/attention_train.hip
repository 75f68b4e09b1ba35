// The fp32 training attention: flash self attention backward for every head width, its forward with log-sum-exp for the
// widths other than 32 (the 32-wide forward is the sampling kernel of attention.hip), and the short-context
// cross-attention backward.  f32 matrix cores (v_mfma_f32_32x32x2f32), fp32 softmax, flash style: the score matrix is
// recomputed tile by tile from Q, K and the forward's per-row log-sum-exp, never stored.
//   P = exp(scale*QK^T - L),  dV = P^T dO,  dP = dO V^T,  dS = P o (dP - D),  D = rowsum(dO o O),
//   dQ = scale * dS K,  dK = scale * dS^T Q.
// The backward is two kernels, both deterministic (no atomics):
//   attn_bwd_dq_kernel : a wave owns 32 queries and walks the keys   -> dQ
//   attn_bwd_dkv_kernel: a wave owns 32 keys    and walks the queries -> dK, dV
// A 32x32 score tile leaves the MFMA with (column = the wave's own index on the lane, 16 registers x 2 half-waves = the
// other index), which is the k-pair layout of the B operand of the next product, so P and dS feed the following MFMAs
// straight from registers.
// One family of templates on DP = the head width padded to a multiple of 32 (32, 64, 96):
//   * O, dQ, dK, dV are DP/32 accumulators of 16 registers, one per 32-column chunk of the head;
//   * at DP = 64 and 96 the real width d_head (32 < d_head <= DP, a multiple of 4) is a runtime argument: columns >= d_head
//     are masked to 0 in the operand loads and in the tile staging (exact for Q K^T and dO V^T, whose contractions run
//     over DP/2 MFMA steps) and are never stored.  At DP = 32 the width is the constant and every mask folds away.
// LDS: two staged 64 x (DP+1) tiles (16.5 KB at DP = 32, 32.5 KB at 64, 48.5 KB at 96).  At 64 and 96 the per-wave 32 x 33
// transpose buffers of the row stores are aliased onto the staged tiles after a final workgroup barrier, so the static
// 64 KB limit holds; the DP = 32 backward kernels keep buffers of their own (see ALIAS_TS).
#include "ldmk_common.h"

namespace ldmk {

constexpr int AT_T = 64;          // rows per staged tile
constexpr int AT_TS = 32 * 33;    // floats of a wave's transpose buffer (store_rows)

// Backward kernels: do the four transpose buffers reuse the staged tiles?  Not at DP = 32.  There they fill the tiles to
// the last float and need one more workgroup barrier, and on an MI355X (shipped UNet, latent 64, batch 16) the aliased
// dK/dV and dQ kernels took 1.0 % and 0.7 % more time than with buffers of their own, against <= 0.25 % between two runs
// of an unchanged kernel; 33.8 KB of LDS costs no occupancy at 124 / 159 VGPRs.
template <int DP>
constexpr bool ALIAS_TS = DP != 32;

// D[b][h][q] = sum_d dO[q][h][d] * O[q][h][d]
__global__ void attn_rowdot_kernel(const float* __restrict__ dout, const float* __restrict__ out, float* __restrict__ dsum,
                                   int tokens, int heads, int d_head, long long total) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long row = i / heads;
  const int h = (int)(i - row * heads);
  const long long b = row / tokens;
  const int q = (int)(row - b * tokens);
  const float4* a = reinterpret_cast<const float4*>(dout + (row * heads + h) * d_head);
  const float4* o = reinterpret_cast<const float4*>(out + (row * heads + h) * d_head);
  float s = 0.f;
  const int n4 = d_head / 4;
  int j = 0;
  // 32 columns at a time with all 16 loads in flight (a thread's row is its own 128 B lines: one pair per trip took the
  // 32-wide call 2.7x the time, 32.7 against 11.9 us per call in the shipped UNet's step), then the rest; one fmaf order
  for (; j + 8 <= n4; j += 8) {
    float4 x[8], y[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { x[u] = a[j + u]; y[u] = o[j + u]; }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      s = fmaf(x[u].x, y[u].x, s); s = fmaf(x[u].y, y[u].y, s); s = fmaf(x[u].z, y[u].z, s); s = fmaf(x[u].w, y[u].w, s);
    }
  }
  for (; j < n4; ++j) {
    const float4 x = a[j], y = o[j];
    s = fmaf(x.x, y.x, s); s = fmaf(x.y, y.y, s); s = fmaf(x.z, y.z, s); s = fmaf(x.w, y.w, s);
  }
  dsum[(b * heads + h) * tokens + q] = s;
}

// stage 64 rows x DP floats of a [rows][ld] matrix (row r0.., src already at the head's first column) into a
// stride-(DP+1) LDS image (padded rows: one image serves the row-wise and the column-wise operand reads); rows past the
// end and columns past d_head are zeros
template <int DP>
__device__ __forceinline__ void stage_tile(float* dst, const float* __restrict__ src, long long ld, int r0, int rows, int d_head,
                                           int tid) {
  constexpr int C4 = DP / 4, N4 = AT_T * C4 / 256;
  float4 v[N4];
#pragma unroll
  for (int i = 0; i < N4; ++i) {
    const int idx = tid + 256 * i, rr = idx / C4, d4 = (idx - rr * C4) * 4;
    const int r = r0 + rr;
    v[i] = (r < rows && d4 < d_head) ? *reinterpret_cast<const float4*>(src + (long long)r * ld + d4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int i = 0; i < N4; ++i) {
    const int idx = tid + 256 * i, rr = idx / C4, d4 = (idx - rr * C4) * 4;
    float* d = dst + rr * (DP + 1) + d4;
    d[0] = v[i].x; d[1] = v[i].y; d[2] = v[i].z; d[3] = v[i].w;
  }
}

// a lane's DP/2 B-operand values of its row: step s pairs d = 2s (lanes 0-31) with d = 2s + 1 (lanes 32-63).  The row
// pointer is clamped by the caller and mul is 0 for a row past the end: unconditional loads
template <int DP>
__device__ __forceinline__ void load_frag(float (&f)[DP / 2], const float* __restrict__ p, int d_head, int half, float mul) {
#pragma unroll
  for (int s = 0; s < DP / 2; ++s) f[s] = (2 * s + half < d_head) ? p[2 * s + half] * mul : 0.f;
}

// write one 32-column chunk (columns c0..c0+31 of the head) of a wave's accumulator, held as
// acc[r] = X^T[d = c0 + (r&3)+8*(r>>2)+4*half][row = l31], as rows of 128 B; columns >= d_head are not stored
__device__ __forceinline__ void store_rows(float* ts, const f32x16& acc, float mul, float* __restrict__ dst, long long ld,
                                           int row0, int rows, int c0, int d_head, int l31, int half) {
#pragma unroll
  for (int r = 0; r < 16; ++r) ts[l31 * 33 + (r & 3) + 8 * (r >> 2) + 4 * half] = acc[r] * mul;
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
  if (c0 + l31 < d_head) {
#pragma unroll
    for (int q = 0; q < 32; q += 2)
      if (row0 + q + half < rows) dst[(long long)(row0 + q + half) * ld + c0 + l31] = ts[(q + half) * 33 + l31];
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
}

// Forward (DP = 64, 96): out[n*tokens][C], lse[n][heads][tokens] = natural log-sum-exp of the scaled scores.  The 64-key
// tile loop of the backward kernels with an online softmax in the log2 domain.
template <int DP>
__global__ __launch_bounds__(256) void attn_fwd_lse_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                           float* __restrict__ lse, int tokens, int heads, int d_head, float scale) {
  constexpr int STR = DP + 1, NC = DP / 32;
  static_assert(4 * AT_TS <= 2 * AT_T * STR, "the transpose buffers are aliased onto the staged tiles");
  __shared__ float smem[2 * AT_T * STR];
  float* Ks = smem;
  float* Vs = smem + AT_T * STR;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int C = heads * d_head, ld = 3 * C;
  const int h = blockIdx.y, b = blockIdx.z;
  const int q0 = blockIdx.x * 128 + wave * 32;
  const float* base = qkv + (long long)b * tokens * ld;
  const bool wave_active = q0 < tokens;
  const bool q_valid = q0 + l31 < tokens;
  const int qq = q_valid ? q0 + l31 : 0;
  constexpr float LOG2E = 1.4426950408889634f;
  float qf[DP / 2];                                      // pre-scaled by scale * log2(e): scores live in the log2 domain
  load_frag<DP>(qf, base + (long long)qq * ld + h * d_head, d_head, half, q_valid ? scale * LOG2E : 0.f);
  f32x16 o[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[c][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  const int ntiles = (tokens + AT_T - 1) / AT_T;
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();
    stage_tile<DP>(Ks, base + C + h * d_head, ld, kt * AT_T, tokens, d_head, tid);
    stage_tile<DP>(Vs, base + 2 * C + h * d_head, ld, kt * AT_T, tokens, d_head, tid);
    __syncthreads();
    if (!wave_active) continue;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int key0 = kt * AT_T + sub * 32;
      if (key0 >= tokens) break;
      f32x16 sa;
#pragma unroll
      for (int r = 0; r < 16; ++r) sa[r] = 0.f;
      const float* kb = Ks + (sub * 32 + l31) * STR + half;
#pragma unroll
      for (int s = 0; s < DP / 2; ++s) sa = __builtin_amdgcn_mfma_f32_32x32x2f32(kb[2 * s], qf[s], sa, 0, 0, 0);   // S^T[key][q]
      if (key0 + 32 > tokens) {          // last sub-tile of a ragged sequence only (kept a real branch, see attention.hip)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (key0 + (r & 3) + 8 * (r >> 2) + 4 * half >= tokens) sa[r] = -INFINITY;
      }
      float mx = fmaxf(sa[0], sa[1]);
#pragma unroll
      for (int r = 2; r < 16; r += 2) mx = fmaxf(mx, fmaxf(sa[r], sa[r + 1]));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);              // finite: key0 < tokens, so the sub-tile has a real key
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sa[r] = __builtin_amdgcn_exp2f(sa[r] - m_new);
        psum += sa[r];
      }
      psum += __shfl_xor(psum, 32, 64);
      const float corr = __builtin_amdgcn_exp2f(m_run - m_new);     // 0 on the first tile (m_run = -inf)
      l_run = l_run * corr + psum;
      m_run = m_new;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int r = 0; r < 16; ++r) o[c][r] *= corr;
        const float* vc = Vs + (sub * 32 + 4 * half) * STR + 32 * c + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          o[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(vc[((r & 3) + 8 * (r >> 2)) * STR], sa[r], o[c], 0, 0, 0);   // O^T[d][q]
      }
    }
  }
  __syncthreads();                       // every wave is done with the staged tiles: they become the transpose buffers
  if (!wave_active) return;
  if (half == 0 && q_valid) lse[((long long)b * heads + h) * tokens + qq] = (m_run + log2f(l_run)) * 0.6931471805599453f;
  const float inv = 1.0f / l_run;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    store_rows(smem + wave * AT_TS, o[c], inv, out + (long long)b * tokens * C + h * d_head, C, q0, tokens, 32 * c, d_head,
               l31, half);
}

template <int DP>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                          const float* __restrict__ lse, const float* __restrict__ dsum,
                                                          float* __restrict__ dqkv, int tokens, int heads, int d_head,
                                                          float scale) {
  constexpr int STR = DP + 1, NC = DP / 32;
  constexpr int TILES = 2 * AT_T * STR;
  static_assert(!ALIAS_TS<DP> || 4 * AT_TS <= TILES, "the transpose buffers are aliased onto the staged tiles");
  __shared__ float smem[TILES + (ALIAS_TS<DP> ? 0 : 4 * AT_TS)];
  float* Ks = smem;
  float* Vs = smem + AT_T * STR;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  float* ts = smem + (ALIAS_TS<DP> ? 0 : TILES) + wave * AT_TS;
  const int dh = DP == 32 ? DP : d_head;       // at 32 the width is the constant: every mask below folds away
  const int C = heads * dh, ld = 3 * C;
  const int h = blockIdx.y, b = blockIdx.z;
  const int q0 = blockIdx.x * 128 + wave * 32;
  const float* base = qkv + (long long)b * tokens * ld;
  const bool wave_active = q0 < tokens;
  const bool q_valid = q0 + l31 < tokens;
  const int qq = q_valid ? q0 + l31 : 0;
  float qf[DP / 2], dof[DP / 2];
  load_frag<DP>(qf, base + (long long)qq * ld + h * dh, dh, half, q_valid ? scale : 0.f);
  load_frag<DP>(dof, dout + ((long long)b * tokens + qq) * C + h * dh, dh, half, q_valid ? 1.f : 0.f);
  const float Lq = q_valid ? lse[((long long)b * heads + h) * tokens + qq] : INFINITY;
  const float Dq = q_valid ? dsum[((long long)b * heads + h) * tokens + qq] : 0.f;
  f32x16 dq[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[c][r] = 0.f;

  const int ntiles = (tokens + AT_T - 1) / AT_T;
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();
    stage_tile<DP>(Ks, base + C + h * dh, ld, kt * AT_T, tokens, dh, tid);
    stage_tile<DP>(Vs, base + 2 * C + h * dh, ld, kt * AT_T, tokens, dh, tid);
    __syncthreads();
    if (!wave_active) continue;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int key0 = kt * AT_T + sub * 32;
      if (key0 >= tokens) break;
      f32x16 sa, da;
#pragma unroll
      for (int r = 0; r < 16; ++r) { sa[r] = 0.f; da[r] = 0.f; }
      const float* kb = Ks + (sub * 32 + l31) * STR + half;
      const float* vb = Vs + (sub * 32 + l31) * STR + half;
#pragma unroll
      for (int s = 0; s < DP / 2; ++s) {
        sa = __builtin_amdgcn_mfma_f32_32x32x2f32(kb[2 * s], qf[s], sa, 0, 0, 0);     // S^T[key][q]
        da = __builtin_amdgcn_mfma_f32_32x32x2f32(vb[2 * s], dof[s], da, 0, 0, 0);    // dP^T[key][q]
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) sa[r] = __expf(sa[r] - Lq);
      if (key0 + 32 > tokens) {          // last sub-tile of a ragged sequence only (kept a real branch, see attention.hip)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (key0 + (r & 3) + 8 * (r >> 2) + 4 * half >= tokens) sa[r] = 0.f;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) sa[r] *= da[r] - Dq;                                 // dS^T[key][q]
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const float* kc = Ks + (sub * 32 + 4 * half) * STR + 32 * c + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          dq[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(kc[((r & 3) + 8 * (r >> 2)) * STR], sa[r], dq[c], 0, 0, 0);   // dQ^T[d][q]
      }
    }
  }
  if constexpr (ALIAS_TS<DP>) __syncthreads();          // the staged tiles become the transpose buffers
  if (!wave_active) return;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    store_rows(ts, dq[c], scale, dqkv + (long long)b * tokens * ld + h * dh, ld, q0, tokens, 32 * c, dh, l31,
               half);
}

template <int DP>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                           const float* __restrict__ lse, const float* __restrict__ dsum,
                                                           float* __restrict__ dqkv, int tokens, int heads, int d_head,
                                                           float scale) {
  constexpr int STR = DP + 1, NC = DP / 32;
  constexpr int TILES = 2 * AT_T * STR;
  static_assert(!ALIAS_TS<DP> || 4 * AT_TS <= TILES, "the transpose buffers are aliased onto the staged tiles");
  __shared__ float smem[TILES + (ALIAS_TS<DP> ? 0 : 4 * AT_TS)];
  __shared__ float Ls[AT_T], Ds[AT_T];
  float* Qs = smem;
  float* Os = smem + AT_T * STR;            // dO tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  float* ts = smem + (ALIAS_TS<DP> ? 0 : TILES) + wave * AT_TS;
  const int dh = DP == 32 ? DP : d_head;       // at 32 the width is the constant: every mask below folds away
  const int C = heads * dh, ld = 3 * C;
  const int h = blockIdx.y, b = blockIdx.z;
  const int k0 = blockIdx.x * 128 + wave * 32;
  const float* base = qkv + (long long)b * tokens * ld;
  const float* dbase = dout + (long long)b * tokens * C;
  const bool wave_active = k0 < tokens;
  const bool k_valid = k0 + l31 < tokens;
  const int kk = k_valid ? k0 + l31 : 0;
  float kf[DP / 2], vf[DP / 2];
  load_frag<DP>(kf, base + (long long)kk * ld + C + h * dh, dh, half, k_valid ? scale : 0.f);
  load_frag<DP>(vf, base + (long long)kk * ld + 2 * C + h * dh, dh, half, k_valid ? 1.f : 0.f);
  f32x16 dk[NC], dv[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[c][r] = 0.f; dv[c][r] = 0.f; }
  const float* lrow = lse + ((long long)b * heads + h) * tokens;
  const float* drow = dsum + ((long long)b * heads + h) * tokens;

  const int ntiles = (tokens + AT_T - 1) / AT_T;
  for (int qt = 0; qt < ntiles; ++qt) {
    __syncthreads();
    stage_tile<DP>(Qs, base + h * dh, ld, qt * AT_T, tokens, dh, tid);
    stage_tile<DP>(Os, dbase + h * dh, C, qt * AT_T, tokens, dh, tid);
    if (tid < AT_T) {
      const int q = qt * AT_T + tid;
      Ls[tid] = q < tokens ? lrow[q] : INFINITY;       // exp(s - inf) = 0: rows past the end contribute nothing
      Ds[tid] = q < tokens ? drow[q] : 0.f;
    }
    __syncthreads();
    if (!wave_active) continue;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int qbase = qt * AT_T + sub * 32;
      if (qbase >= tokens) break;
      f32x16 sa, da;
#pragma unroll
      for (int r = 0; r < 16; ++r) { sa[r] = 0.f; da[r] = 0.f; }
      const float* qb = Qs + (sub * 32 + l31) * STR + half;
      const float* ob = Os + (sub * 32 + l31) * STR + half;
#pragma unroll
      for (int s = 0; s < DP / 2; ++s) {
        sa = __builtin_amdgcn_mfma_f32_32x32x2f32(qb[2 * s], kf[s], sa, 0, 0, 0);     // S[q][key]
        da = __builtin_amdgcn_mfma_f32_32x32x2f32(ob[2 * s], vf[s], da, 0, 0, 0);     // dP[q][key]
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ql = sub * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        const float p = __expf(sa[r] - Ls[ql]);
        da[r] = p * (da[r] - Ds[ql]);      // dS[q][key]
        sa[r] = p;                         // P[q][key]
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const float* oc = Os + (sub * 32 + 4 * half) * STR + 32 * c + l31;
        const float* qc = Qs + (sub * 32 + 4 * half) * STR + 32 * c + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int o = ((r & 3) + 8 * (r >> 2)) * STR;
          dv[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(oc[o], sa[r], dv[c], 0, 0, 0);          // dV^T[d][key] += dO^T P
          dk[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(qc[o], da[r], dk[c], 0, 0, 0);          // dK^T[d][key] += Q^T dS
        }
      }
    }
  }
  if constexpr (ALIAS_TS<DP>) __syncthreads();          // the staged tiles become the transpose buffers
  if (!wave_active) return;
  float* obase = dqkv + (long long)b * tokens * ld + h * dh;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    store_rows(ts, dk[c], scale, obase + C, ld, k0, tokens, 32 * c, dh, l31, half);
    store_rows(ts, dv[c], 1.0f, obase + 2 * C, ld, k0, tokens, 32 * c, dh, l31, half);
  }
}

template <int DP>
static void launch_self_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, float* dsum,
                            int n, int tokens, int heads, int d_head, float scale, hipStream_t st) {
  const long long total = (long long)n * tokens * heads;
  // (at DP = 32 only the row-dot kernel reads d_head: the other two take the width from the template argument)
  hipLaunchKernelGGL(attn_rowdot_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dout, out, dsum, tokens, heads,
                     d_head, total);
  dim3 grid((tokens + 127) / 128, heads, n);
  hipLaunchKernelGGL(attn_bwd_dq_kernel<DP>, grid, dim3(256), 0, st, qkv, dout, lse, dsum, dqkv, tokens, heads, d_head, scale);
  hipLaunchKernelGGL(attn_bwd_dkv_kernel<DP>, grid, dim3(256), 0, st, qkv, dout, lse, dsum, dqkv, tokens, heads, d_head, scale);
}


// ---------------------------------------------------------------------------------------------------------------
// Backward of the short-context cross attention at head width D (ldmk_attn_cross / ldmk_attn_cross_d, L <= 128 keys;
// attention.py:170-193 with a context).
// Pass 1, one thread per (row, head): recompute p over the L keys, dP_j = dO.v_j, dS_j = p_j (dP_j - sum_i p_i dP_i)
// * scale, dQ = sum_j dS_j k_j; p and dS are kept ([rows][heads][L]) for pass 2.
template <int D>
__global__ __launch_bounds__(256) void attn_cross_bwd_q_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                               const float* __restrict__ v, int ldkv,
                                                               const float* __restrict__ dout, int ldo, float* __restrict__ dq,
                                                               float* __restrict__ pbuf, float* __restrict__ dsbuf, int tokens,
                                                               int L, int heads, float scale, long long total) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // (sample, token, head)
  if (idx >= total) return;
  const int h = (int)(idx % heads);
  const long long row = idx / heads;
  const int b = (int)(row / tokens);
  float qv[D], dov[D], dqv[D];
  const float* qp = q + row * ldq + h * D;
  const float* dp_ = dout + row * ldo + h * D;
#pragma unroll
  for (int d = 0; d < D; ++d) { qv[d] = qp[d]; dov[d] = dp_[d]; dqv[d] = 0.f; }
  const float* kb = k + (long long)b * L * ldkv + h * D;
  const float* vb = v + (long long)b * L * ldkv + h * D;
  float* pr = pbuf + idx * L;
  float* dsr = dsbuf + idx * L;
  float m = -INFINITY;
  for (int j = 0; j < L; ++j) {                        // scores (kept in pbuf), running max
    const float* kp = kb + (long long)j * ldkv;
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) s = fmaf(qv[d], kp[d], s);
    s *= scale;
    pr[j] = s;
    m = fmaxf(m, s);
  }
  float l = 0.f;
  for (int j = 0; j < L; ++j) { const float e = __expf(pr[j] - m); pr[j] = e; l += e; }
  const float inv = 1.0f / l;
  float dsum = 0.f;
  for (int j = 0; j < L; ++j) {                        // p, dP (kept in dsbuf), D = sum p dP
    const float* vp = vb + (long long)j * ldkv;
    float dpj = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) dpj = fmaf(dov[d], vp[d], dpj);
    const float pj = pr[j] * inv;
    pr[j] = pj;
    dsr[j] = dpj;
    dsum = fmaf(pj, dpj, dsum);
  }
  for (int j = 0; j < L; ++j) {
    const float ds = pr[j] * (dsr[j] - dsum) * scale;
    dsr[j] = ds;
    const float* kp = kb + (long long)j * ldkv;
#pragma unroll
    for (int d = 0; d < D; ++d) dqv[d] = fmaf(ds, kp[d], dqv[d]);
  }
  float* dqp = dq + row * ldq + h * D;
#pragma unroll
  for (int d = 0; d < D; ++d) dqp[d] = dqv[d];
}

// Pass 2, one wave per (sample, key, head): dK[j] = sum_q dS[q][j] q[q], dV[j] = sum_q p[q][j] dO[q]; lanes split the
// queries, D values per lane folded with a wave reduction (fixed order).
template <int D>
__global__ __launch_bounds__(256) void attn_cross_bwd_kv_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ dout,
                                                                int ldo, const float* __restrict__ pbuf,
                                                                const float* __restrict__ dsbuf, float* __restrict__ dk,
                                                                float* __restrict__ dv, int ldkv, int tokens, int L, int heads,
                                                                long long total) {
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);          // (sample, key, head)
  if (w >= total) return;
  const int lane = threadIdx.x & 63;
  const int h = (int)(w % heads);
  const long long r = w / heads;
  const int j = (int)(r % L), b = (int)(r / L);
  float ak[D], av[D];
#pragma unroll
  for (int d = 0; d < D; ++d) { ak[d] = 0.f; av[d] = 0.f; }
  for (int t = lane; t < tokens; t += 64) {
    const long long row = (long long)b * tokens + t;
    const float ds = dsbuf[(row * heads + h) * L + j], pj = pbuf[(row * heads + h) * L + j];
    const float* qp = q + row * ldq + h * D;
    const float* dp_ = dout + row * ldo + h * D;
#pragma unroll
    for (int d = 0; d < D; ++d) { ak[d] = fmaf(ds, qp[d], ak[d]); av[d] = fmaf(pj, dp_[d], av[d]); }
  }
  float* dkp = dk + ((long long)b * L + j) * ldkv + h * D;
  float* dvp = dv + ((long long)b * L + j) * ldkv + h * D;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const float sk = wave_sum(ak[d]), sv = wave_sum(av[d]);
    if (lane == 0) { dkp[d] = sk; dvp[d] = sv; }
  }
}

template <int D>
static void launch_cross_bwd(const float* q, int ldq, const float* k, const float* v, int ldkv, const float* dout, int ldo,
                             float* dq, float* dk, float* dv, float* scratch, int n, int tokens, int ctx_len, int heads,
                             float scale, hipStream_t st) {
  const long long total = (long long)n * tokens * heads;
  float* pbuf = scratch;                              // [n*tokens][heads][L]
  float* dsbuf = scratch + total * ctx_len;
  hipLaunchKernelGGL(attn_cross_bwd_q_kernel<D>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, q, ldq, k, v, ldkv, dout,
                     ldo, dq, pbuf, dsbuf, tokens, ctx_len, heads, scale, total);
  const long long waves = (long long)n * ctx_len * heads;
  hipLaunchKernelGGL(attn_cross_bwd_kv_kernel<D>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, q, ldq, dout, ldo, pbuf,
                     dsbuf, dk, dv, ldkv, tokens, ctx_len, heads, waves);
}

}  // namespace ldmk

extern "C" int ldmk_attn_self_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                                  float* dsum, int n, int tokens, int heads, float scale, void* stream) {
  LDMK_ENTER();
  using namespace ldmk;
  LDMK_REQUIRE(qkv && out && dout && lse && dqkv && dsum, "ldmk_attn_self_bwd: null buffer");
  LDMK_REQUIRE(n > 0 && tokens > 0 && heads > 0 && heads <= 65535 && n <= 65535, "ldmk_attn_self_bwd: bad shape");
  launch_self_bwd<32>(qkv, out, dout, lse, dqkv, dsum, n, tokens, heads, 32, scale, (hipStream_t)stream);
  return check_launch("ldmk_attn_self_bwd");
}

extern "C" int ldmk_attn_cross_bwd(const float* q, int ldq, const float* k, const float* v, int ldkv, const float* dout, int ldo,
                                   float* dq, float* dk, float* dv, float* scratch, int n, int tokens, int ctx_len, int heads,
                                   float scale, void* stream) {
  LDMK_ENTER();
  using namespace ldmk;
  LDMK_REQUIRE(q && k && v && dout && dq && dk && dv && scratch, "ldmk_attn_cross_bwd: null buffer");
  LDMK_REQUIRE(n > 0 && tokens > 0 && heads > 0 && ctx_len >= 1 && ctx_len <= 128, "ldmk_attn_cross_bwd: bad shape (ctx_len in [1,128])");
  launch_cross_bwd<32>(q, ldq, k, v, ldkv, dout, ldo, dq, dk, dv, scratch, n, tokens, ctx_len, heads, scale, (hipStream_t)stream);
  return check_launch("ldmk_attn_cross_bwd");
}

#define LDMK_ATTN_D_SHAPE(name)                                                                                              \
  LDMK_REQUIRE(n > 0 && tokens > 0 && heads > 0 && heads <= 65535 && n <= 65535, name ": bad shape");                        \
  LDMK_REQUIRE(d_head > 32 && d_head <= 96 && d_head % 4 == 0,                                                               \
               name ": head width %d (a multiple of 4 in (32, 96]; 32 has its own entry point)", d_head)

extern "C" int ldmk_attn_self_lse_d(const float* qkv, float* out, float* lse, int n, int tokens, int heads, int d_head,
                                    float scale, void* stream) {
  LDMK_ENTER();
  using namespace ldmk;
  LDMK_REQUIRE(qkv && out && lse, "ldmk_attn_self_lse_d: null buffer");
  LDMK_ATTN_D_SHAPE("ldmk_attn_self_lse_d");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((tokens + 127) / 128, heads, n);
  if (d_head <= 64)
    hipLaunchKernelGGL(attn_fwd_lse_kernel<64>, grid, dim3(256), 0, st, qkv, out, lse, tokens, heads, d_head, scale);
  else
    hipLaunchKernelGGL(attn_fwd_lse_kernel<96>, grid, dim3(256), 0, st, qkv, out, lse, tokens, heads, d_head, scale);
  return check_launch("ldmk_attn_self_lse_d");
}

extern "C" int ldmk_attn_self_bwd_d(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                                    float* dsum, int n, int tokens, int heads, int d_head, float scale, void* stream) {
  LDMK_ENTER();
  using namespace ldmk;
  LDMK_REQUIRE(qkv && out && dout && lse && dqkv && dsum, "ldmk_attn_self_bwd_d: null buffer");
  LDMK_ATTN_D_SHAPE("ldmk_attn_self_bwd_d");
  hipStream_t st = (hipStream_t)stream;
  if (d_head <= 64) launch_self_bwd<64>(qkv, out, dout, lse, dqkv, dsum, n, tokens, heads, d_head, scale, st);
  else launch_self_bwd<96>(qkv, out, dout, lse, dqkv, dsum, n, tokens, heads, d_head, scale, st);
  return check_launch("ldmk_attn_self_bwd_d");
}

extern "C" int ldmk_attn_cross_bwd_d(const float* q, int ldq, const float* k, const float* v, int ldkv, const float* dout, int ldo,
                                     float* dq, float* dk, float* dv, float* scratch, int n, int tokens, int ctx_len, int heads,
                                     int d_head, float scale, void* stream) {
  LDMK_ENTER();
  using namespace ldmk;
  LDMK_REQUIRE(q && k && v && dout && dq && dk && dv && scratch, "ldmk_attn_cross_bwd_d: null buffer");
  LDMK_REQUIRE(n > 0 && tokens > 0 && heads > 0 && ctx_len >= 1 && ctx_len <= 128, "ldmk_attn_cross_bwd_d: bad shape (ctx_len in [1,128])");
  hipStream_t st = (hipStream_t)stream;
#define LDMK_XB(D) launch_cross_bwd<D>(q, ldq, k, v, ldkv, dout, ldo, dq, dk, dv, scratch, n, tokens, ctx_len, heads, scale, st)
  switch (d_head) {
    case 40: LDMK_XB(40); break;
    case 64: LDMK_XB(64); break;
    case 80: LDMK_XB(80); break;
    default: LDMK_REQUIRE(false, "ldmk_attn_cross_bwd_d: head width %d (built: 40, 64, 80; 32 has its own entry point)", d_head);
  }
#undef LDMK_XB
  return check_launch("ldmk_attn_cross_bwd_d");
}
