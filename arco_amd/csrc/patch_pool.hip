// The patch-wise pooling of the stage-1 output heads (arco_amd/stage1.py patch_heads(route="gpu"), pretrain_2D / pretrain_3D --patch_heads gpu):
//   arco_patch_pool_fwd   x [B, C, n...] -> y [P, B, C, pool...]: adaptive average pooling of every patch of the patch / 2-stride grid
//   arco_patch_pool_bwd   gy [P, B, C, pool...] -> gx [B, C, n...]: its adjoint, as a gather
// The geometry (patch grid, cell windows, patch numbering) is patch_geom.h's, shared with patch_head.hip.
//
// One thread per output element, plain loops, no atomics and no cross-lane sums: two runs give the same bits.  Every float operation
// rounds on its own (no fused multiply-add), so that tests/patch_pool_refs.py can state the arithmetic element by element.
#pragma clang fp contract(off)
#include "patch_geom.h"

namespace {

// y[p, b, c, i0, i1, i2] = (sum of the window, axis 0 outermost, every axis ascending, starting from 0.f) / (float)(window elements)
__global__ __launch_bounds__(PP_THREADS) void patch_pool_fwd_kernel(const float* __restrict__ x, Geom g, long total, float* __restrict__ y) {
  const Axis a0 = g.a[0], a1 = g.a[1], a2 = g.a[2];
  for (long u = (long)blockIdx.x * PP_THREADS + threadIdx.x; u < total; u += (long)gridDim.x * PP_THREADS) {
    long r = u;
    const int i2 = (int)(r % a2.pool); r /= a2.pool;
    const int i1 = (int)(r % a1.pool); r /= a1.pool;
    const int i0 = (int)(r % a0.pool); r /= a0.pool;
    const long bc = r % ((long)g.B * g.C); r /= (long)g.B * g.C;
    const int p2 = (int)(r % a2.np); r /= a2.np;
    const int p1 = (int)(r % a1.np); r /= a1.np;
    const int p0 = (int)r;
    y[u] = window_mean(x + bc * a0.n * a1.n * a2.n, g, cell_window(g, p0, p1, p2, i0, i1, i2));
  }
}

// the patches [p_lo, p_hi] of an axis that cover the coordinate v (none: p_lo > p_hi, the tail behind the last patch)
__device__ __forceinline__ void covering_patches(const Axis& a, int v, int& p_lo, int& p_hi) {
  p_lo = v < a.patch ? 0 : (v - a.patch) / a.step + 1;
  p_hi = min(v / a.step, a.np - 1);
}
// the cells [i_lo, i_hi] of a patch whose window covers the local coordinate l: floor(i * patch / pool) <= l < ceil((i + 1) * patch / pool)
__device__ __forceinline__ void covering_cells(const Axis& a, int l, int& i_lo, int& i_hi) {
  i_lo = (int)((long)l * a.pool / a.patch);
  i_hi = min((int)((((long)l + 1) * a.pool - 1) / a.patch), a.pool - 1);
}

// gx[b, c, v0, v1, v2] = sum of gy[p, b, c, i0, i1, i2] / (float)(elements of cell (i0, i1, i2)) over every (patch, cell) whose window holds
// the voxel.  ORDER of the sum, starting from 0.f: six nested loops, from the outermost p0, i0, p1, i1, p2, i2, every one ascending - per
// axis the covering patches and, inside each patch, its covering cells; axis 0 outermost.  A voxel that no patch covers keeps the 0.f.
__global__ __launch_bounds__(PP_THREADS) void patch_pool_bwd_kernel(const float* __restrict__ gy, Geom g, long total, float* __restrict__ gx) {
  const Axis a0 = g.a[0], a1 = g.a[1], a2 = g.a[2];
  const long BC = (long)g.B * g.C;
  for (long u = (long)blockIdx.x * PP_THREADS + threadIdx.x; u < total; u += (long)gridDim.x * PP_THREADS) {
    long r = u;
    const int v2 = (int)(r % a2.n); r /= a2.n;
    const int v1 = (int)(r % a1.n); r /= a1.n;
    const int v0 = (int)(r % a0.n); r /= a0.n;
    const long bc = r;
    int p0a, p0b, p1a, p1b, p2a, p2b;
    covering_patches(a0, v0, p0a, p0b);
    covering_patches(a1, v1, p1a, p1b);
    covering_patches(a2, v2, p2a, p2b);
    float acc = 0.f;
    for (int p0 = p0a; p0 <= p0b; ++p0) {
      int i0a, i0b; covering_cells(a0, v0 - p0 * a0.step, i0a, i0b);
      for (int i0 = i0a; i0 <= i0b; ++i0) {
        const int len0 = win_hi(a0, i0) - win_lo(a0, i0);
        for (int p1 = p1a; p1 <= p1b; ++p1) {
          int i1a, i1b; covering_cells(a1, v1 - p1 * a1.step, i1a, i1b);
          for (int i1 = i1a; i1 <= i1b; ++i1) {
            const int len1 = win_hi(a1, i1) - win_lo(a1, i1);
            for (int p2 = p2a; p2 <= p2b; ++p2) {
              int i2a, i2b; covering_cells(a2, v2 - p2 * a2.step, i2a, i2b);
              const long p = ((long)p0 * a1.np + p1) * a2.np + p2;
              const float* cell = gy + (((p * BC + bc) * a0.pool + i0) * a1.pool + i1) * a2.pool;
              for (int i2 = i2a; i2 <= i2b; ++i2) {
                const int len2 = win_hi(a2, i2) - win_lo(a2, i2);
                acc += cell[i2] / (float)(len0 * len1 * len2);
              }
            }
          }
        }
      }
    }
    gx[u] = acc;
  }
}

inline unsigned blocks_for(long total) {
  const long b = (total + PP_THREADS - 1) / PP_THREADS;
  return (unsigned)(b > PP_MAX_BLOCKS ? PP_MAX_BLOCKS : b);
}

}  // namespace

extern "C" {
/* x [B, C, n0, n1(, n2)] fp32 contiguous -> y [P, B, C, pool, pool(, pool)] fp32; nd = 2 reads n0, n1 and ignores n2. */
int arco_patch_pool_fwd(const float* x, int nd, int B, int C, int n0, int n1, int n2, int patch, int pool, float* y, void* stream) {
  ARCO_CHECK_ARG(x && y);
  Geom g; long in_elems, out_elems;
  ARCO_CHECK_ARG(make_geom(nd, B, C, n0, n1, n2, patch, pool, g, in_elems, out_elems));
  hipLaunchKernelGGL(patch_pool_fwd_kernel, dim3(blocks_for(out_elems)), dim3(PP_THREADS), 0, as_stream(stream), x, g, out_elems, y);
  return arco_launch_status();
}
/* gy in the layout of y -> gx in the layout of x, every element written (0 where no patch covers the voxel). */
int arco_patch_pool_bwd(const float* gy, int nd, int B, int C, int n0, int n1, int n2, int patch, int pool, float* gx, void* stream) {
  ARCO_CHECK_ARG(gy && gx);
  Geom g; long in_elems, out_elems;
  ARCO_CHECK_ARG(make_geom(nd, B, C, n0, n1, n2, patch, pool, g, in_elems, out_elems));
  hipLaunchKernelGGL(patch_pool_bwd_kernel, dim3(blocks_for(in_elems)), dim3(PP_THREADS), 0, as_stream(stream), gy, g, in_elems, gx);
  return arco_launch_status();
}
}  // extern "C"
