// Evaluation: connected components and the largest one on the device, so a label map can stay there from the arg-max
// to the metrics.  Two kernel families on one union-find:
//   arco_cc_largest        FOREGROUND: every x[v] != 0 is one foreground (what scipy.ndimage.label takes) - the reference's nms
//                          post-processing as test_util.py:11-15 getLargestCC has it (label + bincount + argmax)
//   arco_cc_value_largest  BY VALUE: components of EQUAL values and the largest one of every class - what skimage.measure.label (which the
//                          reference's getLargestCC calls) means for a map of more than two classes, and the "keep the largest component
//                          of each class" post-processing of the multi-class 2-D workloads
// The by-value kernels are up to 8 % slower on binary input (profiles/cc_gpu_notes.md) and need a larger workspace, so the foreground
// family is not expressed through them.
//
//   neighbours   differ by +-1 in at most `connectivity` axes ( = scipy's generate_binary_structure(ndim, connectivity); connectivity ==
//                ndim: 8 neighbours in 2-D, 26 in 3-D ); by value they must also have EQUAL values
//   in range     (by value) 1 <= x[v] <= C - 1 (C = classes, 2..256); everything else - 0, negatives, values >= C - is background
//   labels[v]    0 on background, else 1 + the smallest linear index of v's component                       int32 [D][H][W]
//   largest[v]   (foreground) 1 on the component with the most voxels; of several that large, the one whose first voxel comes first  uint8
//   keep[v]      (by value) 1 where v lies in the component of ITS OWN class with the most voxels; the same tie rule                  uint8
//   info         (foreground) int64 [3]: {number of components, linear index of the winner's first voxel, its voxel count}; {0, -1, 0}
//                without foreground
//                (by value) int64 [C + 1][3]: rows 1..C-1 that triple per class, an absent class {0, -1, 0}; row 0 the same triple over all
//                classes together (all components; the one with the most voxels, ties to the first in memory); row C {voxels with a value
//                outside 0..C-1, linear index of the first of them or -1, 0}
// The tie rule is `labels == argmax(bincount(labels)[1:]) + 1` on scipy's raster-order numbering.  Everything is integer and the result
// does not depend on the order of arrival: the same bits on every run.
//
// Union-find on parent[v] <= v (int32, -1 on background), five launches per family (cc_* foreground, ccv_* by value):
//   1. row      one wave per row ballots the foreground (in-range) bits into words, kept in the workspace for the later passes.
//               cc: every foreground voxel finds the start of its run through clz on the inverted words.  ccv: per word it also ballots
//               the RUN-START bits (in range and first of the row, or a value other than the left neighbour's - the left neighbour of
//               lane 0 is carried over from the word before), writes the class of every voxel as a byte (0 = background), counts the
//               out-of-range values, and finds the run start through clz on the run-start words.  parent[v] = that start
//   2. merge    a voxel unites with its BACKWARD neighbour rows only: the previous row of its plane and - 3-D - the same row and the two
//               rows next to it in the previous plane, as `connectivity` admits (ccv: only with cells of ITS value).  Within a
//               neighbour row it takes the centre cell if that is foreground (has its value), else the left and the right cell; where
//               the voxel to its left (right) is of the same run and sees the same neighbour run, that one unites them and this one
//               does nothing: one union per pair of touching runs.  Union: find both roots, atomicMin the smaller into the larger
//               root's parent, go on from the value the atomic returned.  Links only ever point to smaller indices, so a component's
//               last root is its smallest index whatever the order
//   3. flatten  parent[v] = find(v), labels; every run piece of a ballot word (ccv: it also ends at the next run-start bit) adds its
//               length to count[root]; cc counts the roots here
//   4. choose   each root offers cc_key(count, root) to a 64-bit atomicMax (wave maximum first); ccv: to the atomicMax of its class,
//               where it is also counted - a wave reduces the roots of one class at a time
//   5. mask     largest[v] = parent[v] == winner (ccv: the winner of v's class); info (ccv row 0: the sum and the maximum over the classes)
// Termination: find walks strictly down (parent[v] < v until the root, and links never point up); the larger of the union loop's two
// indices strictly decreases with every atomic that does not end the loop (`old` < a, and the find that follows only goes further
// down), bounded below by 0; the row pass walks at most W / 64 - 1 words, k strictly decreasing.  No wave waits for another one,
// nothing is retried.
//   By value: word 0 always holds a start bit for a run that reaches it (column 0 in range is a run start); the per-class reduction of
//   the choose kernel loses at least the lowest bit of its wave-uniform mask of roots per round, at most 64 rounds; info row 0 is a
//   counted loop over the C classes.
// Visibility (MI355X: per-XCD L2s, per-CU L1s that other CUs' stores never refresh): the merge pass reads parent[] with agent-scope
// relaxed atomic loads (L1 bypassed) and writes it with device-scope atomics only.  It would be correct on stale values as well - an
// older parent is still an ancestor in the finished forest, because whoever overwrites a link re-unites what it cut - but the walks
// would be longer.  The flatten pass writes parent[v] while other threads walk through v: both the old and the new value are
// ancestors, and roots do not change in that pass.
//   By value: every other array (the words, the class bytes) is written in one launch and read in a later one.
#include "common.h"

// ---- shared by the two families ---------------------------------------------------------------------------------------------------------
constexpr int CC_MAXDIM = 4096;            // largest D, H or W
constexpr int CC_ROWS = 4;                 // rows per block of the row-wise passes: one per wave

typedef unsigned long long cc_u64;

__host__ __device__ static inline int cc_nw(int W) { return (W + 63) >> 6; }

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

// bit x of a row's words; 0 outside the row
__device__ __forceinline__ bool cc_bit(const cc_u64* __restrict__ row, int x, int W) {
  return x >= 0 && x < W && ((row[x >> 6] >> (x & 63)) & 1);
}

// The winner key of a root: the larger count wins, of equal counts the smaller root (the first in memory); 0 means "no root"
__device__ __forceinline__ cc_u64 cc_key(unsigned int count, long root) {
  return ((cc_u64)count << 32) | (cc_u64)(0xFFFFFFFFu - (unsigned int)root);
}
__device__ __forceinline__ unsigned int cc_key_root(cc_u64 key) { return 0xFFFFFFFFu - (unsigned int)(key & 0xFFFFFFFFull); }

static inline bool cc_dims_ok(int D, int H, int W) {
  return D >= 1 && H >= 1 && W >= 1 && D <= CC_MAXDIM && H <= CC_MAXDIM && W <= CC_MAXDIM && (long)D * H * W < (1L << 31);
}

// ---- foreground: every non-zero label one foreground --------------------------------------------------------------------------------------
constexpr long CC_HEAD = 16;               // workspace header: uint64 best, uint32 components, pad

struct CcWs {                              // the workspace's parts (all offsets multiples of 8 bytes)
  cc_u64* best;
  unsigned int* ncomp;
  cc_u64* bits;                            // [D * H][nw]
  int* parent;                             // [N]
  unsigned int* count;                     // [N]
};
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
  if (v < N && ws.parent[v] == (int)v) key = cc_key(ws.count[v], v);
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
  const int winner = best ? (int)cc_key_root(best) : -2;           // (-2: no parent[] value)
  if (v < N) largest[v] = ws.parent[v] == winner;
  if (v == 0) {
    info[0] = (int64_t)*ws.ncomp;
    info[1] = best ? (int64_t)winner : -1;
    info[2] = (int64_t)(best >> 32);
  }
}

// ---- by value: components of equal values, the largest one of every class -----------------------------------------------------------------
constexpr int CCV_MAXCLASSES = 256;        // classes are kept as bytes

struct CcvWs {                             // the workspace's parts (all offsets multiples of 8 bytes)
  cc_u64* best;                            // [C]   best[c]: the largest key of class c (best[0] unused)
  unsigned int* ncomp;                     // [C]   components of class c
  unsigned int* oob;                       // [2]   voxels out of range, 0xFFFFFFFF - the first one's index (0: none)
  cc_u64* bits;                            // [D * H][nw]   in range
  cc_u64* start;                           // [D * H][nw]   first cell of a run
  int* parent;                             // [N]
  unsigned int* count;                     // [N]
  unsigned char* cls;                      // [N]   the value of an in-range voxel, 0 on background
};
__host__ __device__ static inline long ccv_head(int C) { return (12L * C + 8 + 7) & ~7L; }
__host__ __device__ static inline CcvWs ccv_ws(void* ws, int D, int H, int W, int C) {
  char* p = static_cast<char*>(ws);
  const long rows = (long)D * H, N = rows * W, words = rows * cc_nw(W) * 8, N4 = ((N + 1) & ~1L) * 4;
  CcvWs o;
  o.best = reinterpret_cast<cc_u64*>(p);
  o.ncomp = reinterpret_cast<unsigned int*>(p + 8L * C);
  o.oob = reinterpret_cast<unsigned int*>(p + 12L * C);
  p += ccv_head(C);
  o.bits = reinterpret_cast<cc_u64*>(p);
  o.start = reinterpret_cast<cc_u64*>(p + words);
  o.parent = reinterpret_cast<int*>(p + 2 * words);
  o.count = reinterpret_cast<unsigned int*>(p + 2 * words + N4);
  o.cls = reinterpret_cast<unsigned char*>(p + 2 * words + 2 * N4);
  return o;
}

// class byte x of a row; 0 (background) outside the row
__device__ __forceinline__ int ccv_cls(const unsigned char* __restrict__ row, int x, int W) { return x >= 0 && x < W ? (int)row[x] : 0; }

// grid ceil(D*H / CC_ROWS)
__global__ __launch_bounds__(256) void ccv_row_kernel(const int64_t* __restrict__ X, long rows, int W, int C, CcvWs ws) {
  __shared__ cc_u64 st[CC_ROWS][CC_MAXDIM / 64];                   // the run-start words of the wave's row
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * CC_ROWS + wave;
  const bool live = row < rows;                                    // (wave-uniform; dead waves still reach the barrier)
  const int nw = cc_nw(W);
  const long base = live ? row * W : 0;
  int carry = 0;                                                   // the class of the last cell of the word before (0: none)
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    const bool in = live && x < W;
    const int64_t val = in ? X[base + x] : 0;
    const bool out = in && (val < 0 || val >= C);
    const int c = (in && val >= 1 && val <= C - 1) ? (int)val : 0;
    const int up = __shfl_up(c, 1, 64);
    const int left = lane == 0 ? carry : up;
    carry = __shfl(c, 63, 64);
    const cc_u64 m = __ballot(c != 0);
    const cc_u64 s = __ballot(c != 0 && c != left);                // (x == 0: left is 0)
    const cc_u64 o = __ballot(out);
    if (in) ws.cls[base + x] = (unsigned char)c;
    if (lane == 0) {
      st[wave][w] = s;
      if (live) {
        ws.bits[row * nw + w] = m;
        ws.start[row * nw + w] = s;
        if (o) {
          atomicAdd(ws.oob, (unsigned int)__popcll(o));
          atomicMax(ws.oob + 1, 0xFFFFFFFFu - (unsigned int)(base + w * 64 + __ffsll((long long)o) - 1));
        }
      }
    }
  }
  __syncthreads();
  if (!live) return;
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    if (x >= W) break;
    ws.count[base + x] = 0;
    if (ws.cls[base + x] == 0) {                                   // (this thread's own store)
      ws.parent[base + x] = -1;
      continue;
    }
    const int b = x & 63;
    cc_u64 m = st[wave][w] & (~0ull >> (63 - b));                  // run starts at or left of x
    int k = w;
    while (m == 0 && k > 0) m = st[wave][--k];                     // across words in which the run goes on
    const int start = m ? k * 64 + 63 - __clzll((long long)m) : 0; // the nearest run start
    ws.parent[base + x] = (int)(base + start);
  }
}

// One neighbour row (class bytes nc, run-start words ns, linear index of its first voxel nbase) of the voxel v = (this row, column x) of
// class c; mc / ms are this row's class bytes and run-start words.
__device__ __forceinline__ void ccv_merge_row(int* parent, const unsigned char* __restrict__ mc, const cc_u64* __restrict__ ms,
                                              const unsigned char* __restrict__ nc, const cc_u64* __restrict__ ns, int v, int nbase, int c,
                                              int x, int W, bool diag) {
  const bool run_l = !cc_bit(ms, x, W);                            // x - 1 belongs to this voxel's run (x itself is in range)
  if (ccv_cls(nc, x, W) == c) {
    if (!(run_l && !cc_bit(ns, x, W))) cc_unite(parent, v, nbase + x);        // else x - 1 sees the same two runs
  } else if (diag) {
    const bool run_r = ccv_cls(mc, x + 1, W) == c && !cc_bit(ms, x + 1, W);   // x + 1 belongs to this voxel's run
    if (!run_l && ccv_cls(nc, x - 1, W) == c) cc_unite(parent, v, nbase + x - 1);       // (else x - 1 has that cell above it)
    if (!run_r && ccv_cls(nc, x + 1, W) == c) cc_unite(parent, v, nbase + x + 1);
  }
}

// grid ceil(D*H / CC_ROWS); conn = connectivity (1..3)
__global__ __launch_bounds__(256) void ccv_merge_kernel(int D, int H, int W, int conn, CcvWs ws) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long rows = (long)D * H, row = (long)blockIdx.x * CC_ROWS + wave;
  if (row >= rows) return;
  const int z = (int)(row / H), y = (int)(row % H);
  const int nw = cc_nw(W);
  const unsigned char* __restrict__ mc = ws.cls + row * W;
  const cc_u64* __restrict__ ms = ws.start + row * nw;
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    if (x >= W) break;
    const int c = mc[x];
    if (c == 0) continue;
    const int v = (int)(row * W + x);
    if (y > 0) ccv_merge_row(ws.parent, mc, ms, mc - W, ms - nw, v, (int)((row - 1) * W), c, x, W, conn >= 2);
    if (z > 0) {
      const long up = row - H;                                     // the same row of the previous plane
      ccv_merge_row(ws.parent, mc, ms, ws.cls + up * W, ws.start + up * nw, v, (int)(up * W), c, x, W, conn >= 2);
      if (conn >= 2) {
        if (y > 0) ccv_merge_row(ws.parent, mc, ms, ws.cls + (up - 1) * W, ws.start + (up - 1) * nw, v, (int)((up - 1) * W), c, x, W, conn >= 3);
        if (y < H - 1) ccv_merge_row(ws.parent, mc, ms, ws.cls + (up + 1) * W, ws.start + (up + 1) * nw, v, (int)((up + 1) * W), c, x, W, conn >= 3);
      }
    }
  }
}

// grid ceil(D*H / CC_ROWS)
__global__ __launch_bounds__(256) void ccv_flatten_kernel(long rows, int W, CcvWs ws, int* __restrict__ labels) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * CC_ROWS + wave;
  if (row >= rows) return;
  const int nw = cc_nw(W);
  for (int w = 0; w < nw; ++w) {
    const int x = w * 64 + lane;
    if (x >= W) break;
    const long v = row * W + x;
    const cc_u64 m = ws.bits[row * nw + w], s = ws.start[row * nw + w];
    if (!((m >> lane) & 1)) {
      labels[v] = 0;
      continue;
    }
    const int r = cc_find<false>(ws.parent, (int)v);
    ws.parent[v] = r;
    labels[v] = r + 1;
    if (lane == 0 || ((s >> lane) & 1)) {                          // first cell of a run piece within this word: add the piece's length
      const cc_u64 stop = lane == 63 ? 0 : ((~m | s) >> (lane + 1));          // background or the next run's start (past the row: background)
      const int len = stop ? __ffsll((long long)stop) : 64 - lane;
      atomicAdd(ws.count + r, (unsigned int)len);
    }
  }
}

// grid ceil(N / 256)
__global__ __launch_bounds__(256) void ccv_choose_kernel(long N, CcvWs ws) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool root = v < N && ws.parent[v] == (int)v;               // (background: parent = -1)
  const int c = root ? (int)ws.cls[v] : 0;
  const cc_u64 mine = root ? cc_key(ws.count[v], v) : 0;
  cc_u64 todo = __ballot(root);                                    // wave-uniform; one class per round, its lowest root leads
  while (todo) {
    const int lc = __shfl(c, __ffsll((long long)todo) - 1, 64);
    const bool in = root && c == lc;
    const cc_u64 sub = __ballot(in);
    cc_u64 key = in ? mine : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const cc_u64 other = __shfl_xor(key, o, 64);
      key = other > key ? other : key;
    }
    if (lane == 0) {
      atomicAdd(ws.ncomp + lc, (unsigned int)__popcll(sub));
      atomicMax(ws.best + lc, key);
    }
    todo &= ~sub;                                                  // sub holds todo's lowest bit
  }
}

// grid ceil(N / 256)
__global__ __launch_bounds__(256) void ccv_mask_kernel(long N, int C, CcvWs ws, unsigned char* __restrict__ keep, int64_t* __restrict__ info) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v < N) {
    const int c = ws.cls[v];
    const cc_u64 best = c ? ws.best[c] : 0;                        // (c != 0: the class has a root, best != 0)
    keep[v] = c != 0 && ws.parent[v] == (int)cc_key_root(best);
  }
  if (blockIdx.x != 0) return;
  const int t = threadIdx.x;
  if (t >= 1 && t < C) {
    const cc_u64 best = ws.best[t];
    info[3 * t + 0] = (int64_t)ws.ncomp[t];
    info[3 * t + 1] = best ? (int64_t)cc_key_root(best) : -1;
    info[3 * t + 2] = (int64_t)(best >> 32);
  }
  if (t == 0) {
    cc_u64 best = 0;
    int64_t n = 0;
    for (int c = 1; c < C; ++c) {
      const cc_u64 b = ws.best[c];
      best = b > best ? b : best;
      n += (int64_t)ws.ncomp[c];
    }
    info[0] = n;
    info[1] = best ? (int64_t)cc_key_root(best) : -1;
    info[2] = (int64_t)(best >> 32);
    const unsigned int first = ws.oob[1];
    info[3 * C + 0] = (int64_t)ws.oob[0];
    info[3 * C + 1] = first ? (int64_t)(0xFFFFFFFFu - first) : -1;
    info[3 * C + 2] = 0;
  }
}

static inline bool ccv_classes_ok(int C) { return C >= 2 && C <= CCV_MAXCLASSES; }

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

// bytes of the workspace of arco_cc_value_largest: header (per-class best and counts, the out-of-range record), the rows' in-range and
// run-start words, parent, count and the class bytes; -1 for sizes the launch rejects
long arco_cc_value_ws_bytes(int D, int H, int W, int classes) {
  if (!cc_dims_ok(D, H, W) || !ccv_classes_ok(classes)) return -1;
  const long rows = (long)D * H, N = rows * W;
  return ccv_head(classes) + 2 * rows * cc_nw(W) * 8 + 2 * ((N + 1) & ~1L) * 4 + ((N + 7) & ~7L);
}

int arco_cc_value_largest(const int64_t* x, int D, int H, int W, int ndim, int connectivity, int classes, void* ws, long ws_bytes,
                          int32_t* labels, long labels_bytes, uint8_t* keep, long keep_bytes, int64_t* info, long info_bytes, void* stream) {
  ARCO_CHECK_ARG(x && ws && labels && keep && info);
  ARCO_CHECK_ARG(cc_dims_ok(D, H, W));
  ARCO_CHECK_ARG(ccv_classes_ok(classes));
  ARCO_CHECK_ARG(ndim == 2 || ndim == 3);
  ARCO_CHECK_ARG(ndim == 3 || D == 1);
  ARCO_CHECK_ARG(connectivity >= 1 && connectivity <= ndim);
  const long rows = (long)D * H, N = rows * W;
  ARCO_CHECK_ARG(ws_bytes >= arco_cc_value_ws_bytes(D, H, W, classes));
  ARCO_CHECK_ARG(labels_bytes >= N * (long)sizeof(int32_t) && keep_bytes >= N && info_bytes >= 3 * (classes + 1L) * (long)sizeof(int64_t));
  ARCO_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0);
  hipStream_t st = as_stream(stream);
  const CcvWs w = ccv_ws(ws, D, H, W, classes);
  if (hipMemsetAsync(ws, 0, (size_t)ccv_head(classes), st) != hipSuccess) return ARCO_ERR_LAUNCH;
  const dim3 by_row((unsigned)((rows + CC_ROWS - 1) / CC_ROWS)), by_voxel((unsigned)((N + 255) / 256));
  hipLaunchKernelGGL(ccv_row_kernel, by_row, dim3(256), 0, st, x, rows, W, classes, w);
  hipLaunchKernelGGL(ccv_merge_kernel, by_row, dim3(256), 0, st, D, H, W, connectivity, w);
  hipLaunchKernelGGL(ccv_flatten_kernel, by_row, dim3(256), 0, st, rows, W, w, labels);
  hipLaunchKernelGGL(ccv_choose_kernel, by_voxel, dim3(256), 0, st, N, w);
  hipLaunchKernelGGL(ccv_mask_kernel, by_voxel, dim3(256), 0, st, N, classes, w, keep, info);
  return arco_launch_status();
}

}  // extern "C"
