// Interpolation arithmetic shared by every kernel that resamples: the resize kernels (elementwise.hip), the row gathers of the
// row-sparse heads (det_scatter.hip) and the upsampling GEMM epilogue (gemm_sp.hip).  Each helper is ONE fixed chain of operations,
// so those kernels agree bit for bit whatever the surrounding code lets the compiler contract.
#pragma once
#include "common.h"

// The 8-corner trilinear blend.  Written as the plain expression `hz * (...) + lz * (...)`, the instruction scheduler chose which
// product of each sum became the fma: the fused epilogue differed from the resize kernel in 1-2 ulp on 80 % of the elements.
__device__ __forceinline__ float tl_blend1(float v000, float v001, float v010, float v011, float v100, float v101, float v110, float v111,
                                           float hx, float lx, float hy, float ly, float hz, float lz) {
  const float a0 = __builtin_fmaf(lx, v001, hx * v000), a1 = __builtin_fmaf(lx, v011, hx * v010);
  const float a2 = __builtin_fmaf(lx, v101, hx * v100), a3 = __builtin_fmaf(lx, v111, hx * v110);
  const float b0 = __builtin_fmaf(ly, a1, hy * a0), b1 = __builtin_fmaf(ly, a3, hy * a2);
  return __builtin_fmaf(lz, b1, hz * b0);
}

// The 4-corner bilinear blend of the 2-D kernels (dense resize, row gather, 4-way lerp of the row-sparse heads).  As a plain
// expression the three kernels compiled to three different chains: the gather's rows differed from the dense resize in the last bit
// on 0.5 % of the elements, the lerp's from the gather's on 14 %.  Contraction is off inside, so the two plain products stay products.
__device__ __forceinline__ float bl_blend1(float v00, float v01, float v10, float v11, float hx, float lx, float hy, float ly) {
#pragma clang fp contract(off)
  const float a0 = __builtin_fmaf(lx, v01, hx * v00), a1 = __builtin_fmaf(lx, v11, hx * v10);
  return __builtin_fmaf(ly, a1, hy * a0);
}

// align_corners source index / weight (torch's upsample index math in fp32).  Contraction is off: `src - i0` must subtract from the
// ROUNDED product, as torch's CPU kernel does.  Left to -ffp-contract=fast the compiler fused it into fma(scale, o, -i0) in some
// kernels and not in others, and the interpolation weights came out one ulp apart.
__device__ __forceinline__ void ac_src(int o, float scale, int in_size, int& i0, int& i1, float& l1) {
#pragma clang fp contract(off)
  const float src = scale * (float)o;
  i0 = (int)src; if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 < in_size - 1 ? i0 + 1 : i0;
  l1 = src - (float)i0;
}
