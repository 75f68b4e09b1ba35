// Operand helpers shared by the matrix-core kernels: the 16-bit vector types, the exact splits of an fp32 value into bf16 / fp16
// images (LDMK_COMPUTE_BF16X3 / LDMK_COMPUTE_F16X2, include/ldmk.h), the F16X2 range check and scale, raw buffer descriptors,
// counted waits and the compile-time loop.  One definition each: the split arithmetic is a bitwise contract between the kernels
// that stage an operand themselves and the producers that write it pre-split.
#pragma once
#include "ldmk_common.h"
#include <type_traits>

namespace ldmk {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

__device__ __forceinline__ bf16x4 to_bf16x4(const float4& v) {          // round-to-nearest-even (v_cvt_pk_bf16_f32)
  return bf16x4{(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
}

// exact three-way split x = hi + mid + lo (each difference below is exact in fp32: the subtrahend is the leading part of x)
__device__ __forceinline__ void split3(const float4& v, bf16x4& h, bf16x4& m, bf16x4& l) {
  h = to_bf16x4(v);
  const float4 r = make_float4(v.x - (float)h[0], v.y - (float)h[1], v.z - (float)h[2], v.w - (float)h[3]);
  m = to_bf16x4(r);
  l = to_bf16x4(make_float4(r.x - (float)m[0], r.y - (float)m[1], r.z - (float)m[2], r.w - (float)m[3]));
}

// LDMK_COMPUTE_F16X2: x' = 2^6 x = hi + lo, hi = fp16(x'), lo = fp16(x' - hi) (round-to-nearest-even; x' - hi exact in fp32)
constexpr float H2_SCALE = 64.f;              // 2^LDMK_F16X2_A_EXP
__device__ __forceinline__ void split2h(const float4& v, f16x4& h, f16x4& l) {     // v already scaled; lo: h2_lo_pair (ldmk_common.h)
  h = f16x4{(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
  const u32x2 hu = __builtin_bit_cast(u32x2, h);
  l = __builtin_bit_cast(f16x4, u32x2{h2_lo_pair(hu.x, v.x, v.y), h2_lo_pair(hu.y, v.z, v.w)});
}
__device__ __forceinline__ bool h2_out_of_range(float x) {                         // |x| >= LDMK_F16X2_RANGE, inf or NaN
  return (__float_as_uint(x) & 0x7fffffffu) >= 0x447a0000u;       // 1000.0f
}
__device__ __forceinline__ bool h2_out_of_range(const float4& v) {
  return h2_out_of_range(v.x) || h2_out_of_range(v.y) || h2_out_of_range(v.z) || h2_out_of_range(v.w);
}
// (activations, s = 2^6: saturated just inside the range -- h2_clamp, ldmk_common.h; weights, any s: their exponent is chosen at pack time)
__device__ __forceinline__ float4 scaled(const float4& v, float s) { return make_float4(v.x * s, v.y * s, v.z * s, v.w * s); }
__device__ __forceinline__ float4 scaled_sat(const float4& v) {
  return make_float4(h2_clamp(v.x) * H2_SCALE, h2_clamp(v.y) * H2_SCALE, h2_clamp(v.z) * H2_SCALE, h2_clamp(v.w) * H2_SCALE);
}

// raw buffer descriptor as four SGPRs (uniform), for loads written as inline asm; num_records = bytes, offsets beyond it read zeros
__device__ __forceinline__ u32x4 buffer_rsrc(const void* ptr, unsigned bytes) {
  const unsigned long long a = (unsigned long long)ptr;
  u32x4 r;
  r.x = __builtin_amdgcn_readfirstlane((unsigned)a);
  r.y = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32) & 0xFFFFu);
  r.z = __builtin_amdgcn_readfirstlane(bytes);
  r.w = 0x00020000u;
  return r;
}

// all but the N youngest vector-memory operations of this wave are done (inline-asm loads are not counted by the compiler)
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "i"(N) : "memory"); }

}  // namespace ldmk
