// Operand conversion for the matrix cores: the three-term bf16 split of an fp32 value (MMA = 3, igemm.hip) and the f16 / bf16
// roundings of the reduced-precision modes (MMA = 1 / 2).
#pragma once
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// LDS words are written as packed bf16 pairs and read back as MFMA operands: every such type-punned access goes through a
// may_alias type (without it the compiler may assume that the loads cannot see the stores - observed: a B fragment built
// from one repeated dword)
typedef unsigned int u32x2_ma __attribute__((ext_vector_type(2), may_alias));
typedef unsigned int u32x4_ma __attribute__((ext_vector_type(4), may_alias));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bf16x8 lds_bf16x8(const void* p) { return __builtin_bit_cast(bf16x8, u32x4(*reinterpret_cast<const u32x4_ma*>(p))); }

__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ unsigned perm_hi16(unsigned hi, unsigned lo) {      // {hi[31:16], lo[31:16]}
  return __builtin_amdgcn_perm(hi, lo, 0x07060302u);
}
// The activation split: x = t0 + t1 + t2 bit for bit, each term a bf16.  t0 = bf16(x) by the hardware's round-to-nearest conversion of
// a PAIR (its result is the packed LDS word of plane 0); r1 = x - t0 (exact); t1 = the upper 16 bits of r1 (truncation: one v_and);
// t2 = r1 - t1 (exact, at most 8 significant bits: a bf16 value as it stands).  |t1| <= 2^-8 |x|, |t2| < 2^-15 |x|: the three dropped
// cross products are bounded by 2^-23 + 2^-24 of |x||w|, zero-mean.
// Findings of the retired variants:
//  - Rounding every term to nearest (what the weight pack kernels still do) compiles to ~34 instructions per pair against 11 here.  The
//    loader waves of the pipelined kernels share their SIMD's vector issue port with an MFMA wave and were the side the rendezvous
//    waited for (tools/micro/fc_clock.py, profiles/r06_notes.md section 13).
//  - The FIRST term is rounded, not truncated: rounding keeps the remainders zero-mean.  Truncating it too biases every dropped cross
//    product the same way, the bias adds up over K, and the whole V-Net's gradients moved from 0.4 % to 0.9 % (worst tensor 1.4 % ->
//    9 %) off the float64 reference through extra ReLU flips.
//  - An all-round-to-nearest packed-pair form (10 VALU instructions per pair against 14 element-wise) was 21-23 % faster as pure VALU
//    work (tools/micro/split_rate.hip) and changed nothing where it matters: dense GEMM 160.4 vs 159.4 TFLOP/s, the headline step
//    11.17 / 11.56 vs 11.08 / 11.21 ms.  The kernels that split are bound by on-chip operand traffic (profiles/r05_notes.md section 2).
__device__ __forceinline__ void split3_pair_rt(float x0, float x1, unsigned& h0, unsigned& h1, unsigned& h2) {
  h0 = cvt_pk_bf16(x0, x1);
  const float r0 = x0 - __uint_as_float(h0 << 16), r1 = x1 - __uint_as_float(h0 & 0xffff0000u);
  const unsigned u0 = __float_as_uint(r0) & 0xffff0000u, u1 = __float_as_uint(r1) & 0xffff0000u;
  h1 = perm_hi16(u1, u0);
  h2 = perm_hi16(__float_as_uint(r1 - __uint_as_float(u1)), __float_as_uint(r0 - __uint_as_float(u0)));
}
__device__ __forceinline__ void split3_bf16x4(f32x4 v, u32x2& p0, u32x2& p1, u32x2& p2) {
  const float x0 = v[0], x1 = v[1], x2 = v[2], x3 = v[3];
  unsigned a0, a1, a2, c0, c1, c2;
  split3_pair_rt(x0, x1, a0, a1, a2);
  split3_pair_rt(x2, x3, c0, c1, c2);
  p0 = u32x2{a0, c0}; p1 = u32x2{a1, c1}; p2 = u32x2{a2, c2};
}
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f16x4 to_f16x4(f32x4 v) { return __builtin_convertvector(v, f16x4); }
__device__ __forceinline__ s16x4 to_bf16x4(f32x4 v) {
  s16x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) { const __bf16 b = (__bf16)v[e]; r[e] = __builtin_bit_cast(short, b); }
  return r;
}
