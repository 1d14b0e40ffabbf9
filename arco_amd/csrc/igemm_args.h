// Argument block, consumer-side activation loaders, route word and dispatch declarations of the forward / data-gradient
// convolution kernels (igemm.hip, conv_sp.hip, conv3d_fl.hip, gemm_sp.hip, conv_h.hip).
#pragma once
#include <stddef.h>
#include "common.h"

// Flat-position 3x3 tiles (igemm_kernel FLAT, wgrad_halo2_kernel FLAT) stage planes with a padded row stride W + 2 up to this bound
constexpr int IGEMM_FLAT_WPMAX = 64;

// ArcoActPro, the C-ABI descriptor of a consumer-side activation, is include/arco_hip.h's (common.h): the kernels read the caller's
// struct as it is passed, and arco_amd/_lib.py mirrors the same layout for ctypes
static_assert(sizeof(ArcoActPro) == 64 && offsetof(ArcoActPro, seed) == 48, "ArcoActPro: four pointers, four 4-byte scalars, uint64, pointer");

struct IgemmArgs {
  const float* A; long lda;
  const float* Wp; int Npad, Kpad, N, K;
  float* C; long ldc;
  const float* bias;
  const float* R; long ldr;
  float* stat_sum; float* stat_sq;   // [N][n_mblocks] block partials (nullable)
  int n_mblocks; int n_nblocks;
  int NB, H, W;                      // images (planes for 3-D), rows, cols (TAPS==9); TAPS==1 uses M only
  int D3;                            // 3-D: planes per volume (depth taps active when DEPTH==3); 2-D: 1
  long M;                            // total pixels
  int ksplit; long slab_stride;      // split-K (TAPS==1): blockIdx.y = K slab, output slab y at C + y*slab_stride
  int stat_groups;                   // BN groups: images [g*NB/G, (g+1)*NB/G) feed the stat slabs [g*n_mblocks/G, ...)
  int mma;                           // 0: fp32 MFMA (default); 1 / 2: operands rounded to f16 / bf16 in registers, fp32 accumulate (3x3x3, 1x1x1);
                                     // 3: split-bf16; 4: f16 activation STORAGE (A / C are f16 tensors, conv_h.hip)
  int Kg;                            // mma == 3: 16-k groups per packed weight row (= ceil32(K) / 16)
  int batch; long batchA, batchW, batchC;   // TAPS==1 batched GEMM: blockIdx.z = problem, operands at + z * stride (floats)
  // gemm_sp.hip only: the residual is the TRILINEAR (align_corners) upsample of a low-resolution tensor, sampled in the epilogue -
  // FeatureExtractor_3d's `fea_i(cat(up(x), f_i)) + cat(up(x), f_i)` with the wide block pushed under the upsample
  // (model_3D.py:46-58; arco_amd/model_3D.py forward_lowres2): Rup [NV, uD, uH, uW] rows of N channels -> output rows [NV, oD, oH, oW]
  const float* Rup; long ldrup; int uD, uH, uW, oD, oH, oW;
  // Consumer-side activation (pro.mean != nullptr): A holds the PRE-activation z of the producing convolution, and the loader forms
  // a = dropout(lrelu((z - mean) * istd * gamma + beta)) element by element while it stages the tile - the BatchNorm-apply pass
  // between the two convolutions of a block (unetWithArgs.py:36-44, vnetWithArgs.py:16-25) and its HBM round trip are gone.
  // The arithmetic is bn_act_fwd_kernel's, operation for operation: the staged values are bit-identical to the tensor that pass wrote.
  ArcoActPro pro;
};

// the per-channel parameters of four consecutive channels and the prologue applied to one staged quad
struct ProQuad { f32x4 mu, is, ga, be; };
__device__ __forceinline__ f32x4 pro_bn_lrelu(f32x4 z, const ProQuad& q, float slope) {
  f32x4 y;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float v = (z[e] - q.mu[e]) * q.is[e] * q.ga[e] + q.be[e];
    y[e] = v >= 0.f ? v : v * slope;
  }
  return y;
}
// v where keep != 0, +0.0 elsewhere - as a bitwise AND with an all-ones / all-zeros word.  Written `keep ? v : 0` behind the prologue
// arithmetic, hipcc sinks that arithmetic into per-element branches (wgrad_split_kernel<16,16,PRO>: 111 us against 72 us for either
// the arithmetic or the select alone, tools/micro/wgrad_pro_bench.py); the AND keeps the loader straight-line
__device__ __forceinline__ f32x4 pro_mask(f32x4 v, unsigned keep) {
  // (whole-vector bit casts: `__builtin_bit_cast(unsigned, v[e])` on a vector ELEMENT reads element 0 for every e with this clang)
  typedef unsigned int pm_u32x4 __attribute__((ext_vector_type(4)));
  const unsigned m = 0u - (keep & 1u);
  const pm_u32x4 u = __builtin_bit_cast(pm_u32x4, v) & pm_u32x4{m, m, m, m};
  return __builtin_bit_cast(f32x4, u);
}
// nn.Dropout on the quad at element index e0 .. e0 + 3 (element = pixel * C + channel, as bn_act_fwd_kernel counts)
__device__ __forceinline__ f32x4 pro_dropout(f32x4 y, uint32_t key, uint32_t e0, uint32_t thr, float keep_scale) {
  bool keep[4];
  drop_keep_quad(key, e0, thr, keep);
#pragma unroll
  for (int e = 0; e < 4; ++e) y[e] = keep[e] ? y[e] * keep_scale : 0.f;
  return y;
}

// arco_conv_last_route (include/arco_hip.h, test-facing): every launch_* / *_dispatch function notes the id of the kernel it launches -
// the id its query form reports in q[1] - in this per-thread word.  Host side only: one thread-local store per launch.
extern thread_local int arco_last_route;
static inline void arco_note_route(int id) { arco_last_route = id; }

// conv_sp.hip: the software-pipelined split-bf16 3x3 kernel.  Returns -1 when the shape is not one it takes (the caller
// then falls through to igemm_kernel), otherwise the launch status; q != nullptr: query only (q[0] = M-tiles = BN stat
// slabs per channel, q[1] = instantiation id, q[2] = KC*100 + DEPTH*10).
int conv_sp_dispatch(const IgemmArgs& a, hipStream_t st, int* q);
// conv_sp.hip: the resident-weights 3x3x3 kernel of the 16 -> 16 full-resolution level (split-bf16); -1 when the shape is not taken
int conv3d_rw_dispatch(const IgemmArgs& a, hipStream_t st, int* q);
// conv3d_fl.hip: the pipelined flat-tile 3x3x3 kernel of the V-Net levels below full resolution (-1: shape not taken)
int conv3d_fl_dispatch(const IgemmArgs& a, hipStream_t st, int* q);

// gemm_sp.hip: the software-pipelined split-bf16 1x1 GEMM (wide, many-tile launches without BN statistics); -1 when the shape is not taken
int gemm_sp_dispatch(const IgemmArgs& a, hipStream_t st, int* q);

// conv_h.hip: f16 activation storage (mma == 4).  hconv_dispatch: forward / data gradient of the 3x3x3 and 1x1x1 convolutions on
// f16 tensors (a.A, a.C point at f16 rows, a.Wp at the f16 pack [tap][Npad][ceil32(K)], a.Kpad = ceil32(K)); q as above.
int hconv_dispatch(const IgemmArgs& a, int taps, hipStream_t st, int* q);
