// Evaluation: exact surface distances behind hd95 / asd (medpy.metric.binary, restated in utils/metrics.py), on two
// routes that share their passes:
//   arco_surface_hist     unit voxel spacing and connectivity 1 - what the reference always asks for (test_2D.py:52-66,
//                         test_util.py:214-220).  Every squared distance is an integer, so the route is integer arithmetic throughout
//                         and returns a HISTOGRAM of squared distances; the host finishes hd95 / asd from the non-empty bins
//   arco_surface_sp_dist  a voxel spacing and a connectivity: the squared distances are float64, returned one RECORD per border voxel
//
//   border(X)[v] = X[v] and (one neighbour is unset or outside the array); the neighbours are the offsets in {-1, 0, 1}^ndim with 1 to
//                  `connectivity` non-zero components      ( = X ^ binary_erosion(X, generate_binary_structure(ndim, connectivity)) )
//   w_a(e)       = the weight of an offset of e voxels along axis a: e*e (unit), fl(fl(s_a * e) * fl(s_a * e)) (spaced)
//   d2_B[v]      = min over the voxels u of border(B) of fl(fl(w_x(dx) + w_y(dy)) + w_z(dz)),  (dz, dy, dx) = v - u   (2-D: fl(w_x + w_y))
//                  ( unit: distance_transform_edt(~border(B))^2, exactly )
//   hist[c][0][k] = #{v in border(pred == c): d2_{gt == c}[v] == k},   hist[c][1][k] = the same with pred and gt exchanged
//   record        = (val = d2_B[v], tag = (c - c_lo) * 2 + dir) for every v in border(A) with a finite d2_B[v];
//                   dir 0: A = pred == c, B = gt == c; dir 1 the other way round
//
// The two routes are one set of kernels over a metric policy (SfUnit: uint32, SfSpaced: float64 with the axis spacing).  Every float64
// operation is rounded once and none is fused: contraction is off for the file and the products and sums are plain operators (as in
// zoom.hip).  Float64 addition is monotone, so min_x fl(a(x) + b) == fl(min_x a(x) + b) and the separable minimum below IS the d2_B
// above, bit for bit; the minimum is taken with `<` (no NaN arises: every term is >= 0 or +inf).  The unit route has no float, no float
// atomics and nothing that depends on the order of arrival.
//
// Three passes, every class and both directions in one launch each (grid y / z), on two planes of T per (class, direction):
//   1. sf_row_kernel      border bits of a row by wave ballots into LDS; each voxel's nearest set bit to the left and to the right
//                         through clz / ffs on those words -> w_x(d) into plane 0 (inf() where the row has no border voxel)
//   2. sf_minplus_kernel  out(y) = min_y' fl(in(y') + w(y - y')) along H (plane 0 -> 1), then along D (plane 1 -> 0; skipped for ndim 2).
//                         Lanes run across the contiguous axis; the line is staged in LDS as [tile][64] (lane = column), the tile
//                         height such that the tile fills 64 KB: 256 uint32 (lane = bank) or 128 float64 (a lane's 8 bytes sit on the
//                         banks (2 * lane) mod 64, so a 32-lane half covers each once).  Two blocks per CU of 160 KB
//   3. sf_hist_kernel     (unit) every border voxel of A adds one to bin d2_B[v]: the low bins privately in LDS, one 64-bit integer
//                         atomic per non-empty bin and block at the end; the rare large distances go to global integer atomics directly
//      sp_gather_kernel   (spaced) every border voxel of A with a finite d2 appends one record to a packed buffer: a wave counts its
//                         records by ballot, lane 0 moves the 64-bit integer cursor once per wave, each lane writes at its rank.  No
//                         float atomics; nothing is written at or past `cap`, and the cursor ends at the true count.  The order of the
//                         records depends on the order of arrival; their multiset does not (the host sorts them)
// The row pass walks the ballot words to the next non-empty one in a short loop per lane: at most W / 64 - 1 steps each way (63 at the
// largest W, 3 at W = 256), one step at a time only across words without a border voxel; lanes of a wave may leave it at different
// steps.  SF_INF + 4095^2 < 2^31: with dims <= 4096 no unit sum wraps.  A (class, direction) whose B has no border keeps inf()
// everywhere and counts nothing, so a class absent from either map gives two empty histograms and no record.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

constexpr int SF_MAXDIM = 4096;            // largest D, H or W
constexpr int SF_MAXCLS = 32;              // classes per call
constexpr uint32_t SF_INF = 1u << 30;
constexpr int SF_TILE_BYTES = 64 * 1024;   // LDS line tile of the min-plus pass: [SF_TILE_BYTES / (64 * sizeof(T))][64]
constexpr int SF_LOW = 1024;               // privatised low bins of the histogram pass
constexpr int SF_ROWS = 4;                 // rows per block of the row pass: one per wave

typedef unsigned long long sf_u64;

// The metric policies: the element type of the planes, its "no border voxel" value and the weight of an offset along one axis.
struct SfUnit {
  typedef uint32_t T;
  __device__ static T inf() { return SF_INF; }
  __device__ T weight(int e) const { return (uint32_t)(e * e); }
};
struct SfSpaced {
  typedef double T;
  double s;                                // the spacing of the axis the pass runs along
  __device__ static T inf() { return (double)INFINITY; }
  __device__ T weight(int e) const {       // two products, each rounded once
    const double t = s * (double)e;
    return t * t;
  }
};

// v = (z, y, x) is a border voxel of {L == c}.  The neighbour loads happen only where all of them are inside the array.
// CONN: the connectivity as a literal - 1 is the unit route's, the face neighbours written out (the compiler does not fold the loops
// to them) - or 0 for the argument conn
template <int CONN>
__device__ __forceinline__ bool sf_border(const int64_t* __restrict__ L, int64_t c, int z, int y, int x, int D, int H, int W, int ndim,
                                          int conn) {
  const long HW = (long)H * W;
  const long v = (long)z * HW + (long)y * W + x;
  if (L[v] != c) return false;
  bool inside = x > 0 && x < W - 1 && y > 0 && y < H - 1;
  if (ndim == 3) inside = inside && z > 0 && z < D - 1;
  if (!inside) return true;                                        // a face neighbour lies outside at every connectivity
  bool all = true;
  if constexpr (CONN == 1) {
    all = L[v - 1] == c && L[v + 1] == c && L[v - W] == c && L[v + W] == c;
    if (ndim == 3) all = all && L[v - HW] == c && L[v + HW] == c;
  } else {
    const int zr = ndim == 3 ? 1 : 0;
    for (int dz = -zr; dz <= zr; ++dz)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int nz = (dz != 0) + (dy != 0) + (dx != 0);
          if (nz >= 1 && nz <= conn) all = all && L[v + dz * HW + dy * W + dx] == c;
        }
  }
  return !all;
}

// plane p (0 / 1) of pair = cls * 2 + dir; N = D * H * W
template <class T>
__device__ __forceinline__ T* sf_plane(T* ws, long N, int pair, int p) {
  return ws + ((long)pair * 2 + p) * N;
}

// grid (ceil(D*H / SF_ROWS), nc, 2); direction dir measures distances TO border(B), B = gt for dir 0 and pred for dir 1.
// CONN: the connectivity as a literal, or 0 for the argument conn
template <class M, int CONN>
__global__ __launch_bounds__(256) void sf_row_kernel(const int64_t* __restrict__ pred, const int64_t* __restrict__ gt, int D, int H, int W,
                                                    int ndim, int c_lo, typename M::T* __restrict__ ws, int conn, M mx) {
  __shared__ sf_u64 bits[SF_ROWS][SF_MAXDIM / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long rows = (long)D * H, row = (long)blockIdx.x * SF_ROWS + wave;
  const bool live = row < rows;                                    // (wave-uniform; dead waves still reach the barrier)
  const int cls = blockIdx.y, dir = blockIdx.z;
  const int64_t* __restrict__ L = dir == 0 ? gt : pred;
  const int64_t c = (int64_t)c_lo + cls;
  const int z = live ? (int)(row / H) : 0, y = live ? (int)(row % H) : 0;
  const int nw = (W + 63) >> 6;
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    const bool b = live && x < W && sf_border<CONN>(L, c, z, y, x, D, H, W, ndim, conn);
    const sf_u64 m = __ballot(b);
    if (lane == 0) bits[wave][w] = m;
  }
  __syncthreads();
  if (!live) return;
  typename M::T* __restrict__ out = sf_plane(ws, (long)D * H * W, cls * 2 + dir, 0) + row * W;
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    if (x >= W) break;
    const int b = x & 63;
    sf_u64 m = bits[wave][w] & (~0ull >> (63 - b));                // bits 0 .. b: border voxels at or left of x
    int k = w;
    while (m == 0 && k > 0) m = bits[wave][--k];
    int d = m ? x - (k * 64 + 63 - __clzll((long long)m)) : SF_MAXDIM;
    m = bits[wave][w] & (~0ull << b);                              // bits b .. 63: at or right of x
    k = w;
    while (m == 0 && k < nw - 1) m = bits[wave][++k];
    const int dr = m ? k * 64 + __ffsll((long long)m) - 1 - x : SF_MAXDIM;
    d = d < dr ? d : dr;
    out[x] = d >= SF_MAXDIM ? M::inf() : mx.weight(d);
  }
}

// One min-plus pass along a line of Ln entries `inner` apart, for `inner` contiguous columns and gridDim.y outer slices of Ln * inner:
// H pass: Ln = H, inner = W, D slices, m = the y metric; D pass: Ln = D, inner = H * W, one slice, m = the z metric.
// grid (ceil(inner / 64), slices, nc * 2).  64 columns x 4 groups of outputs per block; a thread keeps four outputs in registers per
// candidate read.  Lines longer than the tile take the candidates in chunks; the partial minimum waits in dst meanwhile (written and
// read back by the same thread) - a minimum does not depend on the order its candidates come in.
template <class M>
__global__ __launch_bounds__(256) void sf_minplus_kernel(typename M::T* __restrict__ ws, long N, int from, int to, int Ln, long inner, M m) {
  typedef typename M::T T;
  constexpr int TL = SF_TILE_BYTES / (64 * (int)sizeof(T));
  __shared__ T tile[TL][64];
  const int col = threadIdx.x & 63, g = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + col;
  const bool live = i < inner;
  const long slice = (long)blockIdx.y * Ln * inner;
  const T* __restrict__ src = sf_plane(ws, N, blockIdx.z, from) + slice;
  T* __restrict__ dst = sf_plane(ws, N, blockIdx.z, to) + slice;
  for (int c0 = 0; c0 < Ln; c0 += TL) {
    const int cn = Ln - c0 < TL ? Ln - c0 : TL;
    __syncthreads();                                               // the previous chunk has been read
    for (int t = g; t < cn; t += 4) tile[t][col] = live ? src[(long)(c0 + t) * inner + i] : M::inf();
    __syncthreads();
    if (!live) continue;
    for (int y0 = g; y0 < Ln; y0 += 16) {
      T acc[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int y = y0 + 4 * k;
        acc[k] = (c0 > 0 && y < Ln) ? dst[(long)y * inner + i] : M::inf();
      }
      for (int t = 0; t < cn; ++t) {
        const T v = tile[t][col];
        const int dy = y0 - (c0 + t);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const T s = v + m.weight(dy + 4 * k);
          acc[k] = s < acc[k] ? s : acc[k];
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

// grid (blocks, nc, 2), grid-stride over the voxels; direction dir counts the border voxels of A = pred (dir 0) or gt (dir 1)
__global__ __launch_bounds__(256) void sf_hist_kernel(const int64_t* __restrict__ pred, const int64_t* __restrict__ gt, int D, int H, int W,
                                                     int ndim, int c_lo, uint32_t* __restrict__ ws, int fin, unsigned long long* __restrict__ hist,
                                                     long nbins) {
  __shared__ unsigned int low[SF_LOW];
  for (int k = threadIdx.x; k < SF_LOW; k += 256) low[k] = 0;
  __syncthreads();
  const int cls = blockIdx.y, dir = blockIdx.z;
  const int64_t* __restrict__ A = dir == 0 ? pred : gt;
  const int64_t c = (int64_t)c_lo + cls;
  const long N = (long)D * H * W;
  const uint32_t* __restrict__ d2 = sf_plane(ws, N, cls * 2 + dir, fin);
  unsigned long long* __restrict__ h = hist + (long)(cls * 2 + dir) * nbins;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < N; v += (long)gridDim.x * 256) {
    const int x = (int)(v % W), y = (int)((v / W) % H), z = (int)(v / ((long)W * H));
    if (!sf_border<1>(A, c, z, y, x, D, H, W, ndim, 1)) continue;
    const long b = d2[v];
    if (b >= nbins) continue;                                      // SF_INF: B has no border voxel at all
    if (b < SF_LOW) atomicAdd(&low[b], 1u);
    else atomicAdd(&h[b], 1ull);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < SF_LOW && k < nbins; k += 256)
    if (low[k]) atomicAdd(&h[k], (unsigned long long)low[k]);
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
  const double* __restrict__ d2 = sf_plane(ws, N, cls * 2 + dir, fin);
  for (long v0 = (long)blockIdx.x * 256; v0 < N; v0 += (long)gridDim.x * 256) {
    const long v = v0 + threadIdx.x;
    bool take = false;
    double d = 0.0;
    if (v < N) {
      const int x = (int)(v % W), y = (int)((v / W) % H), z = (int)(v / ((long)W * H));
      if (sf_border<0>(A, c, z, y, x, D, H, W, ndim, conn)) {
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

static inline bool sf_dims_ok(int D, int H, int W) {
  return D >= 1 && H >= 1 && W >= 1 && D <= SF_MAXDIM && H <= SF_MAXDIM && W <= SF_MAXDIM;
}
static inline long sf_nbins(int D, int H, int W) {
  return (long)(D - 1) * (D - 1) + (long)(H - 1) * (H - 1) + (long)(W - 1) * (W - 1) + 1;
}
static inline bool sf_spacing_ok(double s) { return s > 0.0 && s < (double)INFINITY; }      // (false for a NaN)

// what both entry points ask of the maps and the classes; two planes of T per class and direction are the workspace of either
static inline bool sf_args_ok(const void* pred, const void* gt, int D, int H, int W, int ndim, int c_lo, int c_hi) {
  return pred && gt && sf_dims_ok(D, H, W) && (ndim == 2 || ndim == 3) && (ndim == 3 || D == 1) && c_hi >= c_lo &&
         (long)c_hi - c_lo + 1 <= SF_MAXCLS;
}
static inline long sf_ws_bytes(int D, int H, int W, int nc, long elem) {
  if (!sf_dims_ok(D, H, W) || nc < 1 || nc > SF_MAXCLS) return -1;
  return (long)nc * 2 * 2 * D * H * W * elem;
}

// The row pass and the min-plus passes of nc classes from c_lo; the finished d2 lies in plane sf_final(ndim)
template <class M, int CONN>
static void sf_distance_passes(hipStream_t st, const int64_t* pred, const int64_t* gt, int D, int H, int W, int ndim, int conn, int c_lo,
                               int nc, typename M::T* w, M mz, M my, M mx) {
  const long rows = (long)D * H, HW = (long)H * W, N = rows * W;
  hipLaunchKernelGGL((sf_row_kernel<M, CONN>), dim3((unsigned)((rows + SF_ROWS - 1) / SF_ROWS), nc, 2), dim3(256), 0, st, pred, gt, D, H,
                     W, ndim, c_lo, w, conn, mx);
  hipLaunchKernelGGL(sf_minplus_kernel<M>, dim3((unsigned)((W + 63) / 64), D, nc * 2), dim3(256), 0, st, w, N, 0, 1, H, (long)W, my);
  if (ndim == 3) hipLaunchKernelGGL(sf_minplus_kernel<M>, dim3((unsigned)((HW + 63) / 64), 1, nc * 2), dim3(256), 0, st, w, N, 1, 0, D, HW, mz);
}
static inline int sf_final(int ndim) { return ndim == 3 ? 0 : 1; }
static inline unsigned sf_voxel_blocks(long N) { return (unsigned)(N > 1024 * 256 ? 1024 : (N + 255) / 256); }     // grid-stride beyond

extern "C" {

// bytes of the workspace of arco_surface_hist (uint32 planes) / arco_surface_sp_dist (float64 planes); -1 for sizes the launch rejects
long arco_surface_ws_bytes(int D, int H, int W, int nc) { return sf_ws_bytes(D, H, W, nc, (long)sizeof(uint32_t)); }
long arco_surface_sp_ws_bytes(int D, int H, int W, int nc) { return sf_ws_bytes(D, H, W, nc, (long)sizeof(double)); }

// hist[c_hi - c_lo + 1][2][nbins] int64 (zeroed here), nbins = (D-1)^2 + (H-1)^2 + (W-1)^2 + 1
int arco_surface_hist(const int64_t* pred, const int64_t* gt, int D, int H, int W, int ndim, int c_lo, int c_hi, void* ws, long ws_bytes,
                      int64_t* hist, long hist_bytes, void* stream) {
  ARCO_CHECK_ARG(ws && hist && sf_args_ok(pred, gt, D, H, W, ndim, c_lo, c_hi));
  const int nc = c_hi - c_lo + 1;
  const long nbins = sf_nbins(D, H, W), N = (long)D * H * W;
  ARCO_CHECK_ARG(ws_bytes >= arco_surface_ws_bytes(D, H, W, nc));
  ARCO_CHECK_ARG(hist_bytes >= (long)nc * 2 * nbins * (long)sizeof(int64_t));
  hipStream_t st = as_stream(stream);
  uint32_t* w = static_cast<uint32_t*>(ws);
  if (hipMemsetAsync(hist, 0, (size_t)nc * 2 * nbins * sizeof(int64_t), st) != hipSuccess) return ARCO_ERR_LAUNCH;
  sf_distance_passes<SfUnit, 1>(st, pred, gt, D, H, W, ndim, 1, c_lo, nc, w, SfUnit{}, SfUnit{}, SfUnit{});
  hipLaunchKernelGGL(sf_hist_kernel, dim3(sf_voxel_blocks(N), nc, 2), dim3(256), 0, st, pred, gt, D, H, W, ndim, c_lo, w, sf_final(ndim),
                     reinterpret_cast<unsigned long long*>(hist), nbins);
  return arco_launch_status();
}

// val[cap] float64, tag[cap] int32, count[1] int64 (zeroed here): the first min(count, cap) records are written
int arco_surface_sp_dist(const int64_t* pred, const int64_t* gt, int D, int H, int W, int ndim, int connectivity, double sz, double sy,
                         double sx, int c_lo, int c_hi, void* ws, long ws_bytes, double* val, int32_t* tag, long cap, int64_t* count,
                         void* stream) {
  ARCO_CHECK_ARG(ws && val && tag && count && sf_args_ok(pred, gt, D, H, W, ndim, c_lo, c_hi));
  ARCO_CHECK_ARG(connectivity >= 1 && connectivity <= ndim);
  ARCO_CHECK_ARG(sf_spacing_ok(sy) && sf_spacing_ok(sx));
  ARCO_CHECK_ARG(ndim == 2 || sf_spacing_ok(sz));
  const int nc = c_hi - c_lo + 1;
  ARCO_CHECK_ARG(ws_bytes >= arco_surface_sp_ws_bytes(D, H, W, nc));
  ARCO_CHECK_ARG(cap >= 1);
  hipStream_t st = as_stream(stream);
  double* w = static_cast<double*>(ws);
  if (hipMemsetAsync(count, 0, sizeof(int64_t), st) != hipSuccess) return ARCO_ERR_LAUNCH;
  sf_distance_passes<SfSpaced, 0>(st, pred, gt, D, H, W, ndim, connectivity, c_lo, nc, w, SfSpaced{sz}, SfSpaced{sy}, SfSpaced{sx});
  hipLaunchKernelGGL(sp_gather_kernel, dim3(sf_voxel_blocks((long)D * H * W), nc, 2), dim3(256), 0, st, pred, gt, D, H, W, ndim,
                     connectivity, c_lo, w, sf_final(ndim), val, tag, cap, reinterpret_cast<unsigned long long*>(count));
  return arco_launch_status();
}

}  // extern "C"
