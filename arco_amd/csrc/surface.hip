// Evaluation: exact surface distances behind hd95 / asd (medpy.metric.binary, restated in utils/metrics.py) for
// unit voxel spacing and connectivity 1 - what the reference always asks for (test_2D.py:52-66, test_util.py:214-220).
//
//   border(X)[v] = X[v] and (one of the 2*ndim face neighbours is unset or outside the array)    ( = X ^ binary_erosion(X, cross) )
//   d2_B[v]      = squared Euclidean distance from v to the nearest voxel of border(B)           ( = distance_transform_edt(~border(B))^2 )
//   hist[c][0][k] = #{v in border(pred == c): d2_{gt == c}[v] == k},   hist[c][1][k] = the same with pred and gt exchanged
//
// With unit spacing every squared distance is an integer <= (D-1)^2 + (H-1)^2 + (W-1)^2, so the whole file is integer arithmetic:
// no float, no float atomics, nothing that depends on the order of arrival.  The host finishes hd95 / asd from the non-empty bins.
//
// Three passes, every class and both directions in one launch each (grid y / z), on two uint32 planes per (class, direction):
//   1. sf_row_kernel      border bits of a row by wave ballots into LDS; each voxel's nearest set bit to the left and to the right
//                         through clz / ffs on those words -> squared distance along W into plane 0 (SF_INF where the row has no border)
//   2. sf_minplus_kernel  out(y) = min_y' in(y') + (y - y')^2 along H (plane 0 -> 1), then along D (plane 1 -> 0; skipped for ndim 2).
//                         Lanes run across the contiguous axis; the line is staged in LDS as [SF_TL][64] (lane = column = bank)
//   3. sf_hist_kernel     every border voxel of A adds one to bin d2_B[v]: the low bins privately in LDS, one 64-bit integer atomic per
//                         non-empty bin and block at the end; the rare large distances go to global integer atomics directly
// The row pass walks the ballot words to the next non-empty one in a short loop per lane: at most W / 64 - 1 steps each way (63 at the
// largest W, 3 at W = 256), one step at a time only across words without a border voxel; lanes of a wave may leave it at different
// steps.  The min-plus kernel's 64 KB static tile admits two blocks per CU (160 KB of LDS); its lines of up to 256 take one chunk.
// SF_INF + 4095^2 < 2^31: with dims <= 4096 no sum wraps.  A (class, direction) whose B has no border keeps SF_INF everywhere and
// counts nothing, so a class absent from either map gives two empty histograms.
#include "common.h"

constexpr int SF_MAXDIM = 4096;            // largest D, H or W
constexpr int SF_MAXCLS = 32;              // classes per call
constexpr uint32_t SF_INF = 1u << 30;
constexpr int SF_TL = 256;                 // LDS line tile of the min-plus pass (256 x 64 x 4 B = 64 KB)
constexpr int SF_LOW = 1024;               // privatised low bins of the histogram pass
constexpr int SF_ROWS = 4;                 // rows per block of the row pass: one per wave

// v = (z, y, x) is a border voxel of {L == c}.  The neighbour loads happen only where all of them are inside the array.
__device__ __forceinline__ bool sf_border(const int64_t* __restrict__ L, int64_t c, int z, int y, int x, int D, int H, int W, int ndim) {
  const long HW = (long)H * W;
  const long v = (long)z * HW + (long)y * W + x;
  if (L[v] != c) return false;
  bool inside = x > 0 && x < W - 1 && y > 0 && y < H - 1;
  if (ndim == 3) inside = inside && z > 0 && z < D - 1;
  if (!inside) return true;
  bool all = L[v - 1] == c && L[v + 1] == c && L[v - W] == c && L[v + W] == c;
  if (ndim == 3) all = all && L[v - HW] == c && L[v + HW] == c;
  return !all;
}

// plane p (0 / 1) of pair = cls * 2 + dir; N = D * H * W
__device__ __forceinline__ uint32_t* sf_plane(uint32_t* ws, long N, int pair, int p) { return ws + ((long)pair * 2 + p) * N; }

// grid (ceil(D*H / SF_ROWS), nc, 2); direction dir measures distances TO border(B), B = gt for dir 0 and pred for dir 1
__global__ __launch_bounds__(256) void sf_row_kernel(const int64_t* __restrict__ pred, const int64_t* __restrict__ gt, int D, int H, int W,
                                                    int ndim, int c_lo, uint32_t* __restrict__ ws) {
  __shared__ unsigned long long bits[SF_ROWS][SF_MAXDIM / 64];
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
    const bool b = live && x < W && sf_border(L, c, z, y, x, D, H, W, ndim);
    const unsigned long long m = __ballot(b);
    if (lane == 0) bits[wave][w] = m;
  }
  __syncthreads();
  if (!live) return;
  uint32_t* __restrict__ out = sf_plane(ws, (long)D * H * W, cls * 2 + dir, 0) + row * W;
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    if (x >= W) break;
    const int b = x & 63;
    unsigned long long m = bits[wave][w] & (~0ull >> (63 - b));    // bits 0 .. b: border voxels at or left of x
    int k = w;
    while (m == 0 && k > 0) m = bits[wave][--k];
    int d = m ? x - (k * 64 + 63 - __clzll((long long)m)) : SF_MAXDIM;
    m = bits[wave][w] & (~0ull << b);                              // bits b .. 63: at or right of x
    k = w;
    while (m == 0 && k < nw - 1) m = bits[wave][++k];
    const int dr = m ? k * 64 + __ffsll((long long)m) - 1 - x : SF_MAXDIM;
    d = d < dr ? d : dr;
    out[x] = d >= SF_MAXDIM ? SF_INF : (uint32_t)(d * d);
  }
}

// One min-plus pass along a line of Ln entries `inner` apart, for `inner` contiguous columns and gridDim.y outer slices of Ln * inner:
// H pass: Ln = H, inner = W, D slices; D pass: Ln = D, inner = H * W, one slice.  grid (ceil(inner / 64), slices, nc * 2).
// 64 columns x 4 groups of outputs per block; a thread keeps four outputs in registers per candidate read.  Lines longer than the tile
// take the candidates in chunks; the partial minimum waits in dst meanwhile (written and read back by the same thread).
__global__ __launch_bounds__(256) void sf_minplus_kernel(uint32_t* __restrict__ ws, long N, int from, int to, int Ln, long inner) {
  __shared__ uint32_t tile[SF_TL][64];
  const int col = threadIdx.x & 63, g = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * 64 + col;
  const bool live = i < inner;
  const long slice = (long)blockIdx.y * Ln * inner;
  const uint32_t* __restrict__ src = sf_plane(ws, N, blockIdx.z, from) + slice;
  uint32_t* __restrict__ dst = sf_plane(ws, N, blockIdx.z, to) + slice;
  for (int c0 = 0; c0 < Ln; c0 += SF_TL) {
    const int cn = Ln - c0 < SF_TL ? Ln - c0 : SF_TL;
    __syncthreads();                                               // the previous chunk has been read
    for (int t = g; t < cn; t += 4) tile[t][col] = live ? src[(long)(c0 + t) * inner + i] : SF_INF;
    __syncthreads();
    if (!live) continue;
    for (int y0 = g; y0 < Ln; y0 += 16) {
      uint32_t acc[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int y = y0 + 4 * k;
        acc[k] = (c0 > 0 && y < Ln) ? dst[(long)y * inner + i] : SF_INF;
      }
      for (int t = 0; t < cn; ++t) {
        const uint32_t v = tile[t][col];
        const int dy = y0 - (c0 + t);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int e = dy + 4 * k;
          const uint32_t s = v + (uint32_t)(e * e);
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
    if (!sf_border(A, c, z, y, x, D, H, W, ndim)) continue;
    const long b = d2[v];
    if (b >= nbins) continue;                                      // SF_INF: B has no border voxel at all
    if (b < SF_LOW) atomicAdd(&low[b], 1u);
    else atomicAdd(&h[b], 1ull);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < SF_LOW && k < nbins; k += 256)
    if (low[k]) atomicAdd(&h[k], (unsigned long long)low[k]);
}

static inline bool sf_dims_ok(int D, int H, int W) {
  return D >= 1 && H >= 1 && W >= 1 && D <= SF_MAXDIM && H <= SF_MAXDIM && W <= SF_MAXDIM;
}
static inline long sf_nbins(int D, int H, int W) {
  return (long)(D - 1) * (D - 1) + (long)(H - 1) * (H - 1) + (long)(W - 1) * (W - 1) + 1;
}

extern "C" {

// bytes of the workspace of arco_surface_hist: two uint32 planes of D*H*W per class and direction; -1 for sizes the launch rejects
long arco_surface_ws_bytes(int D, int H, int W, int nc) {
  if (!sf_dims_ok(D, H, W) || nc < 1 || nc > SF_MAXCLS) return -1;
  return (long)nc * 2 * 2 * D * H * W * (long)sizeof(uint32_t);
}

// hist[c_hi - c_lo + 1][2][nbins] int64 (zeroed here), nbins = (D-1)^2 + (H-1)^2 + (W-1)^2 + 1
int arco_surface_hist(const int64_t* pred, const int64_t* gt, int D, int H, int W, int ndim, int c_lo, int c_hi, void* ws, long ws_bytes,
                      int64_t* hist, long hist_bytes, void* stream) {
  ARCO_CHECK_ARG(pred && gt && ws && hist);
  ARCO_CHECK_ARG(sf_dims_ok(D, H, W));
  ARCO_CHECK_ARG(ndim == 2 || ndim == 3);
  ARCO_CHECK_ARG(ndim == 3 || D == 1);
  ARCO_CHECK_ARG(c_hi >= c_lo && (long)c_hi - c_lo + 1 <= SF_MAXCLS);
  const int nc = c_hi - c_lo + 1;
  const long nbins = sf_nbins(D, H, W), N = (long)D * H * W;
  ARCO_CHECK_ARG(ws_bytes >= arco_surface_ws_bytes(D, H, W, nc));
  ARCO_CHECK_ARG(hist_bytes >= (long)nc * 2 * nbins * (long)sizeof(int64_t));
  hipStream_t st = as_stream(stream);
  uint32_t* w = static_cast<uint32_t*>(ws);
  if (hipMemsetAsync(hist, 0, (size_t)nc * 2 * nbins * sizeof(int64_t), st) != hipSuccess) return ARCO_ERR_LAUNCH;
  const long rows = (long)D * H;
  hipLaunchKernelGGL(sf_row_kernel, dim3((unsigned)((rows + SF_ROWS - 1) / SF_ROWS), nc, 2), dim3(256), 0, st, pred, gt, D, H, W, ndim,
                     c_lo, w);
  hipLaunchKernelGGL(sf_minplus_kernel, dim3((unsigned)((W + 63) / 64), D, nc * 2), dim3(256), 0, st, w, N, 0, 1, H, (long)W);
  if (ndim == 3) {
    const long HW = (long)H * W;
    hipLaunchKernelGGL(sf_minplus_kernel, dim3((unsigned)((HW + 63) / 64), 1, nc * 2), dim3(256), 0, st, w, N, 1, 0, D, HW);
  }
  long blocks = (N + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(sf_hist_kernel, dim3((unsigned)blocks, nc, 2), dim3(256), 0, st, pred, gt, D, H, W, ndim, c_lo, w, ndim == 3 ? 0 : 1,
                     reinterpret_cast<unsigned long long*>(hist), nbins);
  return arco_launch_status();
}

}  // extern "C"
