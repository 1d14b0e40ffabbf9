// Evaluation: connected components and the largest one - the reference's nms post-processing (test_util.py:11-15
// getLargestCC: skimage.measure.label + bincount + argmax) on the device, so a label map can stay there from the arg-max to the metrics.
//
//   foreground   x[v] != 0 (what scipy.ndimage.label takes); neighbours differ by +-1 in at most `connectivity` axes
//                ( = scipy's generate_binary_structure(ndim, connectivity); connectivity == ndim: 8 neighbours in 2-D, 26 in 3-D )
//   labels[v]    0 on background, else 1 + the smallest linear index of v's component                       int32 [D][H][W]
//   largest[v]   1 on the component with the most voxels; of several that large, the one whose first voxel comes first     uint8
//   info         {number of components, linear index of the winner's first voxel, its voxel count}; {0, -1, 0} without foreground
// That tie rule is `labels == argmax(bincount(labels)[1:]) + 1` on scipy's raster-order numbering.  Everything is integer and the
// result does not depend on the order of arrival: the same bits on every run.
//
// Union-find on parent[v] <= v (int32, -1 on background), five launches:
//   1. cc_row_kernel      one wave per row ballots the foreground bits into words (kept in the workspace for the later passes); every
//                         foreground voxel finds the start of its run through clz on the inverted words: parent[v] = that start
//   2. cc_merge_kernel    a voxel unites with its BACKWARD neighbour rows only: the previous row of its plane and - 3-D - the same
//                         row and the two rows next to it in the previous plane, as `connectivity` admits.  Within a neighbour row it
//                         takes the centre cell if that is foreground, else the left and the right cell; where the voxel to its left
//                         (right) sees the same two runs, that one unites them and this one does nothing: one union per pair of
//                         touching runs.  Union: find both roots, atomicMin the smaller into the larger root's parent, go on from
//                         the value the atomic returned.  Links only ever point to smaller indices, so a component's last root is
//                         its smallest index whatever the order.
//   3. cc_flatten_kernel  parent[v] = find(v), labels; every run piece of a ballot word adds its length to count[root]; roots counted
//   4. cc_choose_kernel   each root offers (count << 32) | (0xFFFFFFFF - root) to one 64-bit atomicMax (wave maximum first)
//   5. cc_mask_kernel     largest[v] = parent[v] == winner; info
// Termination: find walks strictly down (parent[v] < v until the root); the union loop's larger index strictly decreases with every
// atomic; the row pass walks at most W / 64 - 1 words.  No wave waits for another one, nothing is retried.
// Visibility (MI355X: per-XCD L2s, per-CU L1s that other CUs' stores never refresh): the merge pass reads parent[] with agent-scope
// relaxed atomic loads (L1 bypassed) and writes it with device-scope atomics only.  It would be correct on stale values as well - an
// older parent is still an ancestor in the finished forest, because whoever overwrites a link re-unites what it cut - but the walks
// would be longer.  The flatten pass writes parent[v] while other threads walk through v: both the old and the new value are
// ancestors, and roots do not change in that pass.
#include "common.h"

constexpr int CC_MAXDIM = 4096;            // largest D, H or W
constexpr int CC_ROWS = 4;                 // rows per block of the row-wise passes: one per wave
constexpr long CC_HEAD = 16;               // workspace header: uint64 best, uint32 components, pad

typedef unsigned long long cc_u64;

struct CcWs {                              // the workspace's parts (all offsets multiples of 8 bytes)
  cc_u64* best;
  unsigned int* ncomp;
  cc_u64* bits;                            // [D * H][nw]
  int* parent;                             // [N]
  unsigned int* count;                     // [N]
};
__host__ __device__ static inline int cc_nw(int W) { return (W + 63) >> 6; }
__host__ __device__ static inline CcWs cc_ws(void* ws, int D, int H, int W) {
  char* p = static_cast<char*>(ws);
  const long rows = (long)D * H, N = rows * W;
  CcWs o;
  o.best = reinterpret_cast<cc_u64*>(p);
  o.ncomp = reinterpret_cast<unsigned int*>(p + 8);
  o.bits = reinterpret_cast<cc_u64*>(p + CC_HEAD);
  o.parent = reinterpret_cast<int*>(p + CC_HEAD + rows * cc_nw(W) * 8);
  o.count = reinterpret_cast<unsigned int*>(p + CC_HEAD + rows * cc_nw(W) * 8 + ((N + 1) & ~1L) * 4);
  return o;
}

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <bool FRESH>
__device__ __forceinline__ int cc_find(const int* parent, int v) {
  for (;;) {
    const int p = FRESH ? cc_load(parent + v) : parent[v];
    if (p == v) return v;
    v = p;                                                         // p < v: parent[] only points down
  }
}

__device__ __forceinline__ void cc_unite(int* parent, int a, int b) {
  a = cc_find<true>(parent, a);
  b = cc_find<true>(parent, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }                  // a > b
    const int old = atomicMin(parent + a, b);
    if (old == a) break;                                           // a was a root and now hangs under b
    a = cc_find<true>(parent, old);                                // old < a: a's former (or remaining) link; old and b must still meet
    b = cc_find<true>(parent, b);
  }
}

// foreground bit x of a row's words; 0 outside the row
__device__ __forceinline__ bool cc_bit(const cc_u64* __restrict__ row, int x, int W) {
  return x >= 0 && x < W && ((row[x >> 6] >> (x & 63)) & 1);
}

// grid ceil(D*H / CC_ROWS)
__global__ __launch_bounds__(256) void cc_row_kernel(const int64_t* __restrict__ X, long rows, int W, CcWs ws) {
  __shared__ cc_u64 inv[CC_ROWS][CC_MAXDIM / 64];                  // the INVERTED foreground words: set = background
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * CC_ROWS + wave;
  const bool live = row < rows;                                    // (wave-uniform; dead waves still reach the barrier)
  const int nw = cc_nw(W);
  const long base = live ? row * W : 0;
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    const bool f = live && x < W && X[base + x] != 0;
    const cc_u64 m = __ballot(f);
    if (lane == 0) {
      inv[wave][w] = ~m;
      if (live) ws.bits[row * nw + w] = m;
    }
  }
  __syncthreads();
  if (!live) return;
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    if (x >= W) break;
    ws.count[base + x] = 0;
    const int b = x & 63;
    cc_u64 m = inv[wave][w] & (~0ull >> (63 - b));                 // background cells at or left of x
    if (m >> b) {                                                  // x itself is background
      ws.parent[base + x] = -1;
      continue;
    }
    int k = w;
    while (m == 0 && k > 0) m = inv[wave][--k];                    // across words that are all foreground
    const int start = m ? k * 64 + 64 - __clzll((long long)m) : 0; // one past the nearest background cell
    ws.parent[base + x] = (int)(base + start);
  }
}

// One neighbour row nb (linear index of its first voxel nbase) of the voxel v = (row me, column x).
__device__ __forceinline__ void cc_merge_row(int* parent, const cc_u64* __restrict__ me, const cc_u64* __restrict__ nb, int v, int nbase,
                                             int x, int W, bool diag) {
  const bool ml = cc_bit(me, x - 1, W), mr = cc_bit(me, x + 1, W);
  if (cc_bit(nb, x, W)) {
    if (!(ml && cc_bit(nb, x - 1, W))) cc_unite(parent, v, nbase + x);
  } else if (diag) {
    if (!ml && cc_bit(nb, x - 1, W)) cc_unite(parent, v, nbase + x - 1);
    if (!mr && cc_bit(nb, x + 1, W)) cc_unite(parent, v, nbase + x + 1);
  }
}

// grid ceil(D*H / CC_ROWS); conn = connectivity (1..3)
__global__ __launch_bounds__(256) void cc_merge_kernel(int D, int H, int W, int conn, CcWs ws) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long rows = (long)D * H, row = (long)blockIdx.x * CC_ROWS + wave;
  if (row >= rows) return;
  const int z = (int)(row / H), y = (int)(row % H);
  const int nw = cc_nw(W);
  const cc_u64* __restrict__ me = ws.bits + row * nw;
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    if (x >= W || !((me[w] >> lane) & 1)) continue;
    const int v = (int)(row * W + x);
    if (y > 0) cc_merge_row(ws.parent, me, me - nw, v, (int)((row - 1) * W), x, W, conn >= 2);
    if (z > 0) {
      const long up = row - H;                                     // the same row of the previous plane
      cc_merge_row(ws.parent, me, ws.bits + up * nw, v, (int)(up * W), x, W, conn >= 2);
      if (conn >= 2) {
        if (y > 0) cc_merge_row(ws.parent, me, ws.bits + (up - 1) * nw, v, (int)((up - 1) * W), x, W, conn >= 3);
        if (y < H - 1) cc_merge_row(ws.parent, me, ws.bits + (up + 1) * nw, v, (int)((up + 1) * W), x, W, conn >= 3);
      }
    }
  }
}

// grid ceil(D*H / CC_ROWS)
__global__ __launch_bounds__(256) void cc_flatten_kernel(long rows, int W, CcWs ws, int* __restrict__ labels) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * CC_ROWS + wave;
  if (row >= rows) return;
  const int nw = cc_nw(W);
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    if (x >= W) break;
    const long v = row * W + x;
    const cc_u64 m = ws.bits[row * nw + w];
    if (!((m >> lane) & 1)) {
      labels[v] = 0;
      continue;
    }
    const int r = cc_find<false>(ws.parent, (int)v);
    ws.parent[v] = r;
    labels[v] = r + 1;
    if (r == (int)v) atomicAdd(ws.ncomp, 1u);
    if (lane == 0 || !((m >> (lane - 1)) & 1)) {                   // first cell of a run piece within this word: add the piece's length
      const cc_u64 gap = ~(m >> lane);                             // (bit 0 clear; bits past the word's end read as background)
      const int len = gap ? __ffsll((long long)gap) - 1 : 64;
      atomicAdd(ws.count + r, (unsigned int)len);
    }
  }
}

// grid ceil(N / 256)
__global__ __launch_bounds__(256) void cc_choose_kernel(long N, CcWs ws) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  cc_u64 key = 0;
  if (v < N && ws.parent[v] == (int)v) key = ((cc_u64)ws.count[v] << 32) | (cc_u64)(0xFFFFFFFFu - (unsigned int)v);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const cc_u64 other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0 && key) atomicMax(ws.best, key);
}

// grid ceil(N / 256)
__global__ __launch_bounds__(256) void cc_mask_kernel(long N, CcWs ws, unsigned char* __restrict__ largest, int64_t* __restrict__ info) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  const cc_u64 best = *ws.best;
  const int winner = best ? (int)(0xFFFFFFFFu - (unsigned int)(best & 0xFFFFFFFFull)) : -2;       // (-2: no parent[] value)
  if (v < N) largest[v] = ws.parent[v] == winner;
  if (v == 0) {
    info[0] = (int64_t)*ws.ncomp;
    info[1] = best ? (int64_t)winner : -1;
    info[2] = (int64_t)(best >> 32);
  }
}

static inline bool cc_dims_ok(int D, int H, int W) {
  return D >= 1 && H >= 1 && W >= 1 && D <= CC_MAXDIM && H <= CC_MAXDIM && W <= CC_MAXDIM && (long)D * H * W < (1L << 31);
}

extern "C" {

// bytes of the workspace of arco_cc_largest: header, the rows' foreground words, parent and count; -1 for sizes the launch rejects
long arco_cc_ws_bytes(int D, int H, int W) {
  if (!cc_dims_ok(D, H, W)) return -1;
  const long rows = (long)D * H, N = rows * W;
  return CC_HEAD + rows * cc_nw(W) * 8 + ((N + 1) & ~1L) * 4 + N * 4;
}

int arco_cc_largest(const int64_t* x, int D, int H, int W, int ndim, int connectivity, void* ws, long ws_bytes, int32_t* labels,
                    long labels_bytes, uint8_t* largest, long largest_bytes, int64_t* info, long info_bytes, void* stream) {
  ARCO_CHECK_ARG(x && ws && labels && largest && info);
  ARCO_CHECK_ARG(cc_dims_ok(D, H, W));
  ARCO_CHECK_ARG(ndim == 2 || ndim == 3);
  ARCO_CHECK_ARG(ndim == 3 || D == 1);
  ARCO_CHECK_ARG(connectivity >= 1 && connectivity <= ndim);
  const long rows = (long)D * H, N = rows * W;
  ARCO_CHECK_ARG(ws_bytes >= arco_cc_ws_bytes(D, H, W));
  ARCO_CHECK_ARG(labels_bytes >= N * (long)sizeof(int32_t) && largest_bytes >= N && info_bytes >= 3 * (long)sizeof(int64_t));
  ARCO_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0);
  hipStream_t st = as_stream(stream);
  const CcWs w = cc_ws(ws, D, H, W);
  if (hipMemsetAsync(ws, 0, (size_t)CC_HEAD, st) != hipSuccess) return ARCO_ERR_LAUNCH;
  const dim3 by_row((unsigned)((rows + CC_ROWS - 1) / CC_ROWS)), by_voxel((unsigned)((N + 255) / 256));
  hipLaunchKernelGGL(cc_row_kernel, by_row, dim3(256), 0, st, x, rows, W, w);
  hipLaunchKernelGGL(cc_merge_kernel, by_row, dim3(256), 0, st, D, H, W, connectivity, w);
  hipLaunchKernelGGL(cc_flatten_kernel, by_row, dim3(256), 0, st, rows, W, w, labels);
  hipLaunchKernelGGL(cc_choose_kernel, by_voxel, dim3(256), 0, st, N, w);
  hipLaunchKernelGGL(cc_mask_kernel, by_voxel, dim3(256), 0, st, N, w, largest, info);
  return arco_launch_status();
}

}  // extern "C"
