// The geometry of the patch-wise output heads, shared by patch_pool.hip (pooling alone) and patch_head.hip (pooling fused with the
// heads' pointwise layers).  The same on every spatial axis d (nd = 2 or 3): the patches start at 0, step, 2 * step, ... while
// start + patch <= n[d], with step = patch / 2, np[d] = (n[d] - patch) / step + 1 of them; patch number p = (p0 * np[1] + p1) * np[2] + p2
// (the first spatial axis outermost, the heads' loop order).  Cell i of a patch covers the local coordinates
// [floor(i * patch / pool), ceil((i + 1) * patch / pool)), the tensor library's adaptive-pooling windows: they overlap when pool does
// not divide patch, and repeat when pool > patch.  A 2-D call runs the 3-D code with a leading axis of one voxel, one patch and one
// cell of length one: the same sums in the same order.
// Include after `#pragma clang fp contract(off)`: window_mean states its fp32 operations one by one.
#pragma once
#include "common.h"

namespace {

#define PP_THREADS 256
#define PP_MAX_BLOCKS 4096
#define PP_MAX_SIDE 32768            // patch, pool: local coordinate * pool stays inside an int

struct Axis { int n, np, patch, step, pool; };
struct Geom { Axis a[3]; int B, C; };
struct Win { int s0, e0, s1, e1, s2, e2; };      // the voxels [s, e) of a cell's window on the three axes

__host__ __device__ inline int win_lo(const Axis& a, int i) { return (int)((long)i * a.patch / a.pool); }
__host__ __device__ inline int win_hi(const Axis& a, int i) { return (int)(((long)(i + 1) * a.patch + a.pool - 1) / a.pool); }

// the window of cell (i0, i1, i2) of patch (p0, p1, p2)
__device__ __forceinline__ Win cell_window(const Geom& g, int p0, int p1, int p2, int i0, int i1, int i2) {
  Win w;
  w.s0 = p0 * g.a[0].step + win_lo(g.a[0], i0); w.e0 = p0 * g.a[0].step + win_hi(g.a[0], i0);
  w.s1 = p1 * g.a[1].step + win_lo(g.a[1], i1); w.e1 = p1 * g.a[1].step + win_hi(g.a[1], i1);
  w.s2 = p2 * g.a[2].step + win_lo(g.a[2], i2); w.e2 = p2 * g.a[2].step + win_hi(g.a[2], i2);
  return w;
}

// (sum of the window of one [n0, n1, n2] map, axis 0 outermost, every axis ascending, starting from 0.f) / (float)(window elements)
__device__ __forceinline__ float window_mean(const float* __restrict__ src, const Geom& g, const Win& w) {
  float acc = 0.f;
  for (int v0 = w.s0; v0 < w.e0; ++v0)
    for (int v1 = w.s1; v1 < w.e1; ++v1) {
      const float* row = src + ((long)v0 * g.a[1].n + v1) * g.a[2].n;
      for (int v2 = w.s2; v2 < w.e2; ++v2) acc += row[v2];
    }
  return acc / (float)((w.e0 - w.s0) * (w.e1 - w.s1) * (w.e2 - w.s2));
}

// fills g; false for anything the kernels do not take.  in_elems / out_elems: the element counts of [B, C, n...] and [P, B, C, pool...].
inline bool make_geom(int nd, int B, int C, int n0, int n1, int n2, int patch, int pool, Geom& g, long& in_elems, long& out_elems) {
  if ((nd != 2 && nd != 3) || B < 1 || C < 1 || patch < 2 || pool < 1 || patch > PP_MAX_SIDE || pool > PP_MAX_SIDE) return false;
  const int n[3] = {nd == 3 ? n0 : 1, nd == 3 ? n1 : n0, nd == 3 ? n2 : n1};
  const int step = patch / 2;
  __int128 in = (__int128)B * C, out = in;
  for (int d = 0; d < 3; ++d) {
    if (nd == 2 && d == 0) { g.a[d] = Axis{1, 1, 1, 1, 1}; continue; }
    if (n[d] < patch) return false;
    g.a[d] = Axis{n[d], (n[d] - patch) / step + 1, patch, step, pool};
    in *= n[d];
    out *= (__int128)g.a[d].np * pool;
  }
  const __int128 lim = (__int128)1 << 40;          // far above the heads' sizes (4e6 in, 3e6 out); keeps every offset inside a long
  if (in > lim || out > lim || (long)pool * pool * pool > 0x7fffffffL / 2 || (long)patch * patch * patch > 0x7fffffffL / 2) return false;
  g.B = B; g.C = C;
  in_elems = (long)in; out_elems = (long)out;
  return true;
}

}  // namespace
