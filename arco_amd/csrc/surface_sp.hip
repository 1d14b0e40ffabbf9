// Evaluation: the surface distances behind hd95 / asd (medpy.metric.binary, restated in utils/metrics.py) with a
// voxel spacing and a connectivity - the arguments surface.hip leaves to the host.  surface.hip keeps the unit-spacing route and its
// integer histogram; with a spacing the squared distances are real numbers, so this file returns them one RECORD per border voxel:
//
//   border(X)[v] = X[v] and (one neighbour is unset or outside the array); the neighbours are the offsets in {-1, 0, 1}^ndim with 1 to
//                  `connectivity` non-zero components                       ( = X ^ binary_erosion(X, generate_binary_structure(ndim, connectivity)) )
//   w_a(e)       = fl(fl(s_a * e) * fl(s_a * e))                            the float64 weight of an offset of e voxels along axis a
//   d2_B[v]      = min over the voxels u of border(B) of fl(fl(w_x(dx) + w_y(dy)) + w_z(dz)),  (dz, dy, dx) = v - u   (2-D: fl(w_x + w_y))
//   record       = (val = d2_B[v], tag = (c - c_lo) * 2 + dir) for every v in border(A) with a finite d2_B[v];
//                  dir 0: A = pred == c, B = gt == c; dir 1 the other way round
//
// Every float64 operation is rounded once and none is fused: contraction is off for the file and the products and sums are plain
// operators (as in zoom.hip).  Float64 addition is monotone, so min_x fl(a(x) + b) == fl(min_x a(x) + b) and the separable minimum below
// IS the d2_B above, bit for bit; the minimum is taken with `<` (no NaN arises: every term is >= 0 or +inf).
//
// Three passes, every class and both directions in one launch each (grid y / z), on two float64 planes per (class, direction):
//   1. sp_row_kernel      as sf_row_kernel: border bits of a row by wave ballots into LDS, nearest set bit each way through clz / ffs
//                         -> w_x(d) into plane 0, +inf where the row has no border voxel
//   2. sp_minplus_kernel  out(y) = min_y' fl(in(y') + w(|y - y'|)) along H (plane 0 -> 1), then along D (plane 1 -> 0; skipped for
//                         ndim 2).  The line is staged in LDS as [SP_TL][64] float64 (lane = column; 128 x 64 x 8 B = 64 KB, two blocks
//                         per CU of 160 KB); a lane's 8 bytes sit on the banks (2 * lane) mod 64, so a 32-lane half covers each once
//   3. sp_gather_kernel   every border voxel of A with a finite d2 appends one record to a packed buffer: a wave counts its records by
//                         ballot, lane 0 moves the 64-bit integer cursor once per wave, each lane writes at its rank.  No float atomics;
//                         nothing is written at or past `cap`, and the cursor ends at the true count
// The order of the records depends on the order of arrival; their multiset does not (the host sorts them).
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

constexpr int SP_MAXDIM = 4096;            // largest D, H or W
constexpr int SP_MAXCLS = 32;              // classes per call
constexpr int SP_TL = 128;                 // LDS line tile of the min-plus pass (128 x 64 x 8 B = 64 KB)
constexpr int SP_ROWS = 4;                 // rows per block of the row pass: one per wave

// w_a(e): two products, each rounded once
__device__ __forceinline__ double sp_weight(double s, int e) {
  const double t = s * (double)e;
  return t * t;
}

// v = (z, y, x) is a border voxel of {L == c}.  The neighbour loads happen only where all of them are inside the array.
__device__ __forceinline__ bool sp_border(const int64_t* __restrict__ L, int64_t c, int z, int y, int x, int D, int H, int W, int ndim,
                                          int conn) {
  const long HW = (long)H * W;
  const long v = (long)z * HW + (long)y * W + x;
  if (L[v] != c) return false;
  bool inside = x > 0 && x < W - 1 && y > 0 && y < H - 1;
  if (ndim == 3) inside = inside && z > 0 && z < D - 1;
  if (!inside) return true;                                        // a face neighbour lies outside at every connectivity
  const int zr = ndim == 3 ? 1 : 0;
  bool all = true;
  for (int dz = -zr; dz <= zr; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int nz = (dz != 0) + (dy != 0) + (dx != 0);
        if (nz >= 1 && nz <= conn) all = all && L[v + dz * HW + dy * W + dx] == c;
      }
  return !all;
}

// plane p (0 / 1) of pair = cls * 2 + dir; N = D * H * W
__device__ __forceinline__ double* sp_plane(double* ws, long N, int pair, int p) { return ws + ((long)pair * 2 + p) * N; }

// grid (ceil(D*H / SP_ROWS), nc, 2); direction dir measures distances TO border(B), B = gt for dir 0 and pred for dir 1
__global__ __launch_bounds__(256) void sp_row_kernel(const int64_t* __restrict__ pred, const int64_t* __restrict__ gt, int D, int H, int W,
                                                    int ndim, int conn, double sx, int c_lo, double* __restrict__ ws) {
  __shared__ unsigned long long bits[SP_ROWS][SP_MAXDIM / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long rows = (long)D * H, row = (long)blockIdx.x * SP_ROWS + wave;
  const bool live = row < rows;                                    // (wave-uniform; dead waves still reach the barrier)
  const int cls = blockIdx.y, dir = blockIdx.z;
  const int64_t* __restrict__ L = dir == 0 ? gt : pred;
  const int64_t c = (int64_t)c_lo + cls;
  const int z = live ? (int)(row / H) : 0, y = live ? (int)(row % H) : 0;
  const int nw = (W + 63) >> 6;
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    const bool b = live && x < W && sp_border(L, c, z, y, x, D, H, W, ndim, conn);
    const unsigned long long m = __ballot(b);
    if (lane == 0) bits[wave][w] = m;
  }
  __syncthreads();
  if (!live) return;
  double* __restrict__ out = sp_plane(ws, (long)D * H * W, cls * 2 + dir, 0) + row * W;
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    if (x >= W) break;
    const int b = x & 63;
    unsigned long long m = bits[wave][w] & (~0ull >> (63 - b));    // bits 0 .. b: border voxels at or left of x
    int k = w;
    while (m == 0 && k > 0) m = bits[wave][--k];
    int d = m ? x - (k * 64 + 63 - __clzll((long long)m)) : SP_MAXDIM;
    m = bits[wave][w] & (~0ull << b);                              // bits b .. 63: at or right of x
    k = w;
    while (m == 0 && k < nw - 1) m = bits[wave][++k];
    const int dr = m ? k * 64 + __ffsll((long long)m) - 1 - x : SP_MAXDIM;
    d = d < dr ? d : dr;
    out[x] = d >= SP_MAXDIM ? (double)INFINITY : sp_weight(sx, d);
  }
}

// One min-plus pass along a line of Ln entries `inner` apart, for `inner` contiguous columns and gridDim.y outer slices of Ln * inner:
// H pass: Ln = H, inner = W, D slices, s = sy; D pass: Ln = D, inner = H * W, one slice, s = sz.  grid (ceil(inner / 64), slices, nc * 2).
// 64 columns x 4 groups of outputs per block; a thread keeps four outputs in registers per candidate read.  Lines longer than the tile
// take the candidates in chunks; the partial minimum waits in dst meanwhile (written and read back by the same thread) - a minimum
// does not depend on the order its candidates come in.
__global__ __launch_bounds__(256) void sp_minplus_kernel(double* __restrict__ ws, long N, int from, int to, int Ln, long inner, double s) {
  __shared__ double tile[SP_TL][64];
  const int col = threadIdx.x & 63, g = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + col;
  const bool live = i < inner;
  const long slice = (long)blockIdx.y * Ln * inner;
  const double* __restrict__ src = sp_plane(ws, N, blockIdx.z, from) + slice;
  double* __restrict__ dst = sp_plane(ws, N, blockIdx.z, to) + slice;
  const double inf = (double)INFINITY;
  for (int c0 = 0; c0 < Ln; c0 += SP_TL) {
    const int cn = Ln - c0 < SP_TL ? Ln - c0 : SP_TL;
    __syncthreads();                                               // the previous chunk has been read
    for (int t = g; t < cn; t += 4) tile[t][col] = live ? src[(long)(c0 + t) * inner + i] : inf;
    __syncthreads();
    if (!live) continue;
    for (int y0 = g; y0 < Ln; y0 += 16) {
      double acc[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int y = y0 + 4 * k;
        acc[k] = (c0 > 0 && y < Ln) ? dst[(long)y * inner + i] : inf;
      }
      for (int t = 0; t < cn; ++t) {
        const double v = tile[t][col];
        const int dy = y0 - (c0 + t);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double sum = v + sp_weight(s, dy + 4 * k);
          acc[k] = sum < acc[k] ? sum : acc[k];
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int y = y0 + 4 * k;
        if (y < Ln) dst[(long)y * inner + i] = acc[k];
      }
    }
  }
}

// grid (blocks, nc, 2), grid-stride over the voxels in whole waves (every lane of a wave reaches the ballot); direction dir takes the
// border voxels of A = pred (dir 0) or gt (dir 1)
__global__ __launch_bounds__(256) void sp_gather_kernel(const int64_t* __restrict__ pred, const int64_t* __restrict__ gt, int D, int H, int W,
                                                       int ndim, int conn, int c_lo, const double* __restrict__ ws, int fin,
                                                       double* __restrict__ val, int32_t* __restrict__ tag, long cap,
                                                       unsigned long long* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int cls = blockIdx.y, dir = blockIdx.z;
  const int64_t* __restrict__ A = dir == 0 ? pred : gt;
  const int64_t c = (int64_t)c_lo + cls;
  const long N = (long)D * H * W;
  const double* __restrict__ d2 = ws + ((long)(cls * 2 + dir) * 2 + fin) * N;
  for (long v0 = (long)blockIdx.x * 256; v0 < N; v0 += (long)gridDim.x * 256) {
    const long v = v0 + threadIdx.x;
    bool take = false;
    double d = 0.0;
    if (v < N) {
      const int x = (int)(v % W), y = (int)((v / W) % H), z = (int)(v / ((long)W * H));
      if (sp_border(A, c, z, y, x, D, H, W, ndim, conn)) {
        d = d2[v];
        take = d < (double)INFINITY;                               // +inf: B has no border voxel at all
      }
    }
    const unsigned long long m = __ballot(take);
    if (m == 0) continue;                                          // (wave-uniform)
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(count, (unsigned long long)__popcll(m));
    base = __shfl(base, 0);
    const long slot = (long)base + __popcll(m & ((1ull << lane) - 1));
    if (take && slot < cap) {
      val[slot] = d;
      tag[slot] = cls * 2 + dir;
    }
  }
}

static inline bool sp_dims_ok(int D, int H, int W) {
  return D >= 1 && H >= 1 && W >= 1 && D <= SP_MAXDIM && H <= SP_MAXDIM && W <= SP_MAXDIM;
}
static inline bool sp_spacing_ok(double s) { return s > 0.0 && s < (double)INFINITY; }      // (false for a NaN)

extern "C" {

// bytes of the workspace of arco_surface_sp_dist: two float64 planes of D*H*W per class and direction; -1 for sizes the launch rejects
long arco_surface_sp_ws_bytes(int D, int H, int W, int nc) {
  if (!sp_dims_ok(D, H, W) || nc < 1 || nc > SP_MAXCLS) return -1;
  return (long)nc * 2 * 2 * D * H * W * (long)sizeof(double);
}

// val[cap] float64, tag[cap] int32, count[1] int64 (zeroed here): the first min(count, cap) records are written
int arco_surface_sp_dist(const int64_t* pred, const int64_t* gt, int D, int H, int W, int ndim, int connectivity, double sz, double sy,
                         double sx, int c_lo, int c_hi, void* ws, long ws_bytes, double* val, int32_t* tag, long cap, int64_t* count,
                         void* stream) {
  ARCO_CHECK_ARG(pred && gt && ws && val && tag && count);
  ARCO_CHECK_ARG(sp_dims_ok(D, H, W));
  ARCO_CHECK_ARG(ndim == 2 || ndim == 3);
  ARCO_CHECK_ARG(ndim == 3 || D == 1);
  ARCO_CHECK_ARG(connectivity >= 1 && connectivity <= ndim);
  ARCO_CHECK_ARG(sp_spacing_ok(sy) && sp_spacing_ok(sx));
  ARCO_CHECK_ARG(ndim == 2 || sp_spacing_ok(sz));
  ARCO_CHECK_ARG(c_hi >= c_lo && (long)c_hi - c_lo + 1 <= SP_MAXCLS);
  const int nc = c_hi - c_lo + 1;
  const long N = (long)D * H * W;
  ARCO_CHECK_ARG(ws_bytes >= arco_surface_sp_ws_bytes(D, H, W, nc));
  ARCO_CHECK_ARG(cap >= 1);
  hipStream_t st = as_stream(stream);
  double* w = static_cast<double*>(ws);
  if (hipMemsetAsync(count, 0, sizeof(int64_t), st) != hipSuccess) return ARCO_ERR_LAUNCH;
  const long rows = (long)D * H;
  hipLaunchKernelGGL(sp_row_kernel, dim3((unsigned)((rows + SP_ROWS - 1) / SP_ROWS), nc, 2), dim3(256), 0, st, pred, gt, D, H, W, ndim,
                     connectivity, sx, c_lo, w);
  hipLaunchKernelGGL(sp_minplus_kernel, dim3((unsigned)((W + 63) / 64), D, nc * 2), dim3(256), 0, st, w, N, 0, 1, H, (long)W, sy);
  if (ndim == 3) {
    const long HW = (long)H * W;
    hipLaunchKernelGGL(sp_minplus_kernel, dim3((unsigned)((HW + 63) / 64), 1, nc * 2), dim3(256), 0, st, w, N, 1, 0, D, HW, sz);
  }
  long blocks = (N + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(sp_gather_kernel, dim3((unsigned)blocks, nc, 2), dim3(256), 0, st, pred, gt, D, H, W, ndim, connectivity, c_lo, w,
                     ndim == 3 ? 0 : 1, val, tag, cap, reinterpret_cast<unsigned long long*>(count));
  return arco_launch_status();
}

}  // extern "C"
