// The zoom(order=0) round trip of 2-D evaluation (test_2D.py:72-88; arco_amd/eval_surface.py predict_volume(zoom="gpu"),
// arco_amd/utils/zoom_gpu.py): every slice of a volume is resampled to the patch before the network and the arg-max map of the
// network is resampled back to the slice, both by scipy.ndimage.zoom(order=0, mode='constant').
//   zoom_nearest_kernel       [S][n0][n1] -> [S][N0][N1], 4- or 8-byte elements (nearest sampling moves bits: fp32 images, int64 labels)
//   argmax_zoom_back_kernel   logits rows [n * P0 * P1][ld] -> int64 labels [n][x][y]: the class of softmax_rows_kernel (glue.hip) of the
//                             ONE row each output pixel samples; rows no output pixel samples are never read
// and the zoom(order=3) of the image slices that the reference's test.py:124 uses instead (spline_cols_kernel, spline_rows_kernel,
// zoom_cubic_kernel: further down, with their own notes).
// The order-0 kernels are pure streams: a thread writes 16 bytes of consecutive outputs of the fastest axis (one store where the address
// allows it, scalar stores otherwise and at the ragged end of a row), no LDS, no atomics.
//
// The sampling rule is the one of ingest.hip (NI_ZoomShift, order 0): output index o of an axis reads floor(cc + 0.5), cc = o * z in
// float64 with z = (n_in - 1) / (n_out - 1) from the host, and the constant 0 when !(0 <= cc <= n_in - 1) - which happens: for some
// sizes cc of the last index is one ulp above n_in - 1 and the whole last row or column is 0.  A contracted multiply-add would move
// exactly these cases, so contraction is off for the file and the products and sums are plain operators (see ingest.hip).
#pragma clang fp contract(off)
#include <math.h>
#include "common.h"

namespace {

#define ZOOM_MAXC 32             // glue.hip GL_MAXC

// order-0 sample position of output index o on an axis of n points, mode 'constant': false = the constant, else idx in [0, n - 1]
__device__ __forceinline__ bool zoom_index(int o, double z, int n, int& idx) {
  const double cc = (double)o * z;
  if (!(cc >= 0.0 && cc <= (double)(n - 1))) return false;
  idx = (int)floor(cc + 0.5);
  return true;
}

// VEC consecutive elements of T (16 bytes) to p: one store when p is 16-byte aligned and all VEC are inside the row, else one by one
template <typename T, int VEC>
__device__ __forceinline__ void store_run(T* __restrict__ p, const T (&v)[VEC], int valid) {
  typedef T vec_t __attribute__((ext_vector_type(VEC)));
  if (valid == VEC && al16(p)) {
    vec_t w;
#pragma unroll
    for (int e = 0; e < VEC; ++e) w[e] = v[e];
    *reinterpret_cast<vec_t*>(p) = w;
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) if (e < valid) p[e] = v[e];
  }
}

// one thread: the run j0 .. j0 + VEC - 1 of output row (s, i); runs = ceil(N1 / VEC) per row, total = S * N0 * runs
template <typename T>
__global__ __launch_bounds__(256) void zoom_nearest_kernel(const T* __restrict__ src, int n0, int n1, int N0, int N1, int runs, long total,
                                                           double z0, double z1, T* __restrict__ out) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= total) return;
  const long row = q / runs;                       // s * N0 + i
  const int j0 = (int)(q - row * runs) * VEC, i = (int)(row % N0);
  const long s = row / N0;
  T v[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) v[e] = 0;
  int su;
  if (zoom_index(i, z0, n0, su)) {
    const T* line = src + (s * n0 + su) * n1;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      int sv;
      if (j0 + e < N1 && zoom_index(j0 + e, z1, n1, sv)) v[e] = line[sv];
    }
  }
  store_run<T, VEC>(out + row * N1 + j0, v, min(VEC, N1 - j0));
}

// softmax_rows_kernel's `amax` of one logits row: the same expressions in the same order, compiled as glue.hip compiles them (the
// file's contraction switch is undone for this body) - mx by fmaxf, expf(v - mx), the sum in class order, p = e / s and the first
// strict maximum of p.  Not the arg-max of the logits: logits a fraction of an ulp of 1 apart give equal fp32 probabilities.
// f16 rows (T = _Float16; arco_argmax_zoom_back2d_h) are widened to fp32 first - exact, so the class is the one the fp32 kernel gives
// for the fp32 cast of the row -, four classes per 8-byte load where `vec` says that every row allows it, one by one otherwise and at
// the ragged end of a row.
template <typename T>
__device__ __forceinline__ long row_class(const T* __restrict__ x, int C, bool vec) {
#pragma clang fp contract(fast)
  float v[ZOOM_MAXC];
  float mx = -INFINITY;
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int c = 0; c < ZOOM_MAXC; c += 4) {
      if (vec && c + 4 <= C) {
        const f32x4 w = ld4f(x + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[c + e] = w[e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (c + e < C) v[c + e] = (float)x[c + e];
      }
    }
#pragma unroll
    for (int c = 0; c < ZOOM_MAXC; ++c) if (c < C) mx = fmaxf(mx, v[c]);
  } else {
#pragma unroll
    for (int c = 0; c < ZOOM_MAXC; ++c) if (c < C) { v[c] = x[c]; mx = fmaxf(mx, v[c]); }
  }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < ZOOM_MAXC; ++c) if (c < C) { v[c] = expf(v[c] - mx); s += v[c]; }
  float best = -1.f; int bi = 0;
#pragma unroll
  for (int c = 0; c < ZOOM_MAXC; ++c) if (c < C) {
    const float p = v[c] / s;
    if (p > best) { best = p; bi = c; }
  }
  return bi;
}

// one thread: two consecutive labels of output row (s, i); runs = ceil(N1 / 2) per row
template <typename T>
__global__ __launch_bounds__(256) void argmax_zoom_back_kernel(const T* __restrict__ X, long ld, int C, int P0, int P1, int N0, int N1,
                                                               int runs, long total, double z0, double z1, long* __restrict__ out) {
  const bool vec = sizeof(T) == 2 && (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 7) == 0;     // every f16 row starts 8-byte aligned
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= total) return;
  const long row = q / runs;
  const int j0 = (int)(q - row * runs) * 2, i = (int)(row % N0);
  const long s = row / N0;
  long v[2] = {0, 0};
  int su;
  if (zoom_index(i, z0, P0, su)) {
    const T* line = X + (s * P0 + su) * P1 * ld;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      int sv;
      if (j0 + e < N1 && zoom_index(j0 + e, z1, P1, sv)) v[e] = row_class(line + sv * ld, C, vec);
    }
  }
  store_run<long, 2>(out + row * N1 + j0, v, min(2, N1 - j0));
}

// ---- zoom(order=3): scipy's cubic B-spline zoom of a float32 slice, mode 'constant' ----------------------------------------------------
//   spline_cols_kernel / spline_rows_kernel   the float64 prefilter, axis 0 then axis 1 (arco_spline_prefilter2d)
//   zoom_cubic_kernel                          coefficients -> float32 [S][N0][N1] (arco_zoom_cubic2d)
// The bits are the contract (tests/zoom_cubic_kernel_refs.py restates every operation in its order), so a line is filtered strictly in
// sequence - the initial sum over the whole line, the causal recursion, the anticausal recursion: three sweeps, no scan, no
// re-association - and z, the gain and z^(n - 1) are the host's doubles.  With the pole z = sqrt(3) - 2 and c[i] = in[i] * gain:
//   acc = c[0] + zn * c[n-1];  acc += zi * (c[i] + zn * c[n-1-i]), zi *= z  (i = 1 .. n-2, zi = z at i = 1);  c[0] = acc / (1 - zn * zn)
//   c[i] = c[i] + z * c[i-1]  (i = 1 .. n-1);  c[n-1] = (z * c[n-2] + c[n-1]) * z / (z * z - 1);  c[i] = z * (c[i+1] - c[i])  (i = n-2 .. 0)
#define SPL_TC 32                // columns of a row-pass tile
#define SPL_PITCH (SPL_TC + 1)   // its LDS row pitch in doubles: lane r reads 8-byte words 33 r + e, 32 lanes on 32 distinct bank pairs
#define SPL_U 16                 // loads in flight per thread in the column pass

struct SplinePole { double z, gain, zn; };

// axis 0: one thread per (slice, column j), lines of n0 points with stride n1 - neighbouring threads read neighbouring addresses.
// The loads of SPL_U steps are issued together; the arithmetic stays one dependent chain.
__global__ __launch_bounds__(64) void spline_cols_kernel(const float* __restrict__ src, int n0, int n1, long total, SplinePole p,
                                                         double* __restrict__ out) {
  const long q = (long)blockIdx.x * 64 + threadIdx.x;
  if (q >= total) return;
  const long s = q / n1;
  const long off = s * n0 * n1 + (q - s * n1);
  const float* x = src + off;
  double* c = out + off;
  const double z = p.z, gain = p.gain, zn = p.zn;
  const int last = n0 - 1;
  double acc = (double)x[0] * gain + zn * ((double)x[(long)last * n1] * gain);
  double zi = z;
  for (int i0 = 1; i0 < last; i0 += SPL_U) {
    float a[SPL_U], b[SPL_U];
#pragma unroll
    for (int e = 0; e < SPL_U; ++e) {
      const int i = min(i0 + e, last);
      a[e] = x[(long)i * n1];
      b[e] = x[(long)(last - i) * n1];
    }
#pragma unroll
    for (int e = 0; e < SPL_U; ++e) if (i0 + e < last) {
      acc += zi * ((double)a[e] * gain + zn * ((double)b[e] * gain));
      zi *= z;
    }
  }
  acc = acc / (1.0 - zn * zn);
  c[0] = acc;
  double prev = acc, prev2 = acc;
  for (int i0 = 1; i0 <= last; i0 += SPL_U) {
    float a[SPL_U];
#pragma unroll
    for (int e = 0; e < SPL_U; ++e) a[e] = x[(long)min(i0 + e, last) * n1];
#pragma unroll
    for (int e = 0; e < SPL_U; ++e) if (i0 + e <= last) {
      prev2 = prev;
      prev = (double)a[e] * gain + z * prev;
      c[(long)(i0 + e) * n1] = prev;
    }
  }
  double nxt = (z * prev2 + prev) * z / (z * z - 1.0);
  c[(long)last * n1] = nxt;
  for (int i0 = last - 1; i0 >= 0; i0 -= SPL_U) {          // reads what this thread itself wrote
    double a[SPL_U];
#pragma unroll
    for (int e = 0; e < SPL_U; ++e) a[e] = c[(long)max(i0 - e, 0) * n1];
#pragma unroll
    for (int e = 0; e < SPL_U; ++e) if (i0 - e >= 0) {
      nxt = z * (nxt - a[e]);
      c[(long)(i0 - e) * n1] = nxt;
    }
  }
}

// tile <-> global for the row pass: 64 rows x SPL_TC columns, a half-wave per row segment (256 contiguous bytes), two rows per step,
// all 32 steps of a tile in flight at once (the pass waits on memory, not on arithmetic).
// Column e of the tile is column j0 + e of the line, or j0 - e when `rev`.  A fetch of a row >= nr or a column outside [0, n) reads the
// nearest row / column inside instead (no branch in front of a load; those tile cells are never used); such a store is skipped.
#define SPL_STEPS SPL_TC         // steps of a tile transfer: 64 rows, 64 / SPL_TC rows per step
__device__ __forceinline__ void spline_tile_fetch(double (&v)[SPL_STEPS], const double* __restrict__ base, int nr, int n, int j0, bool rev) {
  const int e = threadIdx.x & (SPL_TC - 1), rh = threadIdx.x / SPL_TC;
  const int col = min(max(rev ? j0 - e : j0 + e, 0), n - 1);
#pragma unroll
  for (int k = 0; k < SPL_STEPS; ++k) v[k] = base[(long)min(k * (64 / SPL_TC) + rh, nr - 1) * n + col];
}
__device__ __forceinline__ void spline_tile_put(double* __restrict__ t, const double (&v)[SPL_STEPS]) {
  const int e = threadIdx.x & (SPL_TC - 1), rh = threadIdx.x / SPL_TC;
#pragma unroll
  for (int k = 0; k < SPL_STEPS; ++k) t[(k * (64 / SPL_TC) + rh) * SPL_PITCH + e] = v[k];
}
__device__ __forceinline__ void spline_tile_store(const double* __restrict__ t, double* __restrict__ base, int nr, int n, int j0) {
  const int e = threadIdx.x & (SPL_TC - 1), rh = threadIdx.x / SPL_TC, col = j0 + e;
#pragma unroll
  for (int k = 0; k < SPL_STEPS; ++k) {
    const int r = k * (64 / SPL_TC) + rh;
    if (col < n && r < nr) base[(long)r * n + col] = t[r * SPL_PITCH + e];
  }
}

// axis 1, in place on the coefficients: one wave (= one block) carries 64 rows of n points through LDS tiles of SPL_TC columns - the
// tiles are loaded and stored along the rows, lane r then walks row r of the tile - with the recursion state of its row in registers
// from tile to tile.  The initial sum needs column i and column n - 1 - i at once: a second tile, loaded back to front.  LDS: two
// tiles, whatever n is.  The next tile of a sweep is fetched into registers while the wave walks the current one (a fetch past the
// line's end re-reads its last columns and is dropped).
__global__ __launch_bounds__(64) void spline_rows_kernel(double* __restrict__ c, long rows, int n, SplinePole p) {
  __shared__ double ta[64 * SPL_PITCH], tb[64 * SPL_PITCH];
  const long r0 = (long)blockIdx.x * 64;
  const int nr = (int)min(64L, rows - r0), lane = threadIdx.x;
  const bool live = lane < nr;
  double* base = c + r0 * n;
  double* mine = ta + lane * SPL_PITCH;
  const double* mirror = tb + lane * SPL_PITCH;
  const double z = p.z, gain = p.gain, zn = p.zn;
  const int last = n - 1;
  double va[SPL_STEPS], vb[SPL_STEPS];
  double acc = 0.0, zi = z;
  spline_tile_fetch(va, base, nr, n, 0, false);
  spline_tile_fetch(vb, base, nr, n, last, true);
  for (int j0 = 0; j0 < last; j0 += SPL_TC) {              // the initial sum: i = 0 and i = 1 .. n - 2
    spline_tile_put(ta, va);
    spline_tile_put(tb, vb);
    __syncthreads();
    spline_tile_fetch(va, base, nr, n, j0 + SPL_TC, false);
    spline_tile_fetch(vb, base, nr, n, last - j0 - SPL_TC, true);
    if (live) {
#pragma unroll
      for (int e = 0; e < SPL_TC; ++e) {
        const int i = j0 + e;
        if (i < last) {
          const double v = mine[e] * gain + zn * (mirror[e] * gain);
          if (i == 0) acc = v;
          else { acc += zi * v; zi *= z; }
        }
      }
    }
    __syncthreads();
  }
  acc = acc / (1.0 - zn * zn);
  double prev = acc, prev2 = acc;
  spline_tile_fetch(va, base, nr, n, 0, false);
  for (int j0 = 0; j0 < n; j0 += SPL_TC) {                 // the causal recursion
    spline_tile_put(ta, va);
    __syncthreads();
    spline_tile_fetch(va, base, nr, n, j0 + SPL_TC, false);
    if (live) {
#pragma unroll
      for (int e = 0; e < SPL_TC; ++e) {
        const int i = j0 + e;
        if (i < n) {
          if (i > 0) { prev2 = prev; prev = mine[e] * gain + z * prev; }
          mine[e] = prev;
        }
      }
    }
    __syncthreads();
    spline_tile_store(ta, base, nr, n, j0);
    __syncthreads();                                       // the tile is free again; the stores are visible to the whole wave below
  }
  double nxt = (z * prev2 + prev) * z / (z * z - 1.0);
  spline_tile_fetch(va, base, nr, n, last / SPL_TC * SPL_TC, false);
  for (int j0 = last / SPL_TC * SPL_TC; j0 >= 0; j0 -= SPL_TC) {   // the anticausal recursion, back to front
    spline_tile_put(ta, va);
    __syncthreads();
    spline_tile_fetch(va, base, nr, n, j0 - SPL_TC, false);
    if (live) {
#pragma unroll
      for (int e = SPL_TC - 1; e >= 0; --e) {
        const int i = j0 + e;
        if (i < n) {
          if (i < last) nxt = z * (nxt - mine[e]);
          mine[e] = nxt;
        }
      }
    }
    __syncthreads();
    spline_tile_store(ta, base, nr, n, j0);
    __syncthreads();
  }
}

// one axis of the cubic interpolation at output index o: false = the constant (cc outside [0, n - 1]), else the four taps
// floor(cc) - 1 .. + 2 mirrored into [0, n - 1] (period 2 (n - 1)) and their weights
__device__ __forceinline__ bool cubic_axis(int o, double step, int n, int (&idx)[4], double (&w)[4]) {
  const double cc = (double)o * step;
  if (!(cc >= 0.0 && cc <= (double)(n - 1))) return false;
  const double fl = floor(cc);
  const double x = cc - fl, t = 1.0 - x;
  w[1] = (x * x * (x - 2.0) * 3.0 + 4.0) / 6.0;
  w[2] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
  w[0] = t * t * t / 6.0;
  w[3] = 1.0 - w[0] - w[1] - w[2];
  const int period = 2 * (n - 1), first = (int)fl - 1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int m = (first + k) % period;
    if (m < 0) m += period;
    idx[k] = m > n - 1 ? period - m : m;
  }
  return true;
}

// one thread: the run j0 .. j0 + 3 of output row (s, i); runs = ceil(N1 / 4) per row
__global__ __launch_bounds__(256) void zoom_cubic_kernel(const double* __restrict__ coef, int n0, int n1, int N0, int N1, int runs, long total,
                                                         double z0, double z1, float* __restrict__ out) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= total) return;
  const long row = q / runs;
  const int j0 = (int)(q - row * runs) * 4, i = (int)(row % N0);
  const long s = row / N0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  int ia[4], ib[4];
  double wa[4], wb[4];
  if (cubic_axis(i, z0, n0, ia, wa)) {
    const double* plane = coef + s * n0 * n1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (j0 + e < N1 && cubic_axis(j0 + e, z1, n1, ib, wb)) {
        double t = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const double* line = plane + (long)ia[a] * n1;
#pragma unroll
          for (int b = 0; b < 4; ++b) t += line[ib[b]] * wa[a] * wb[b];
        }
        v[e] = (float)t;
      }
    }
  }
  store_run<float, 4>(out + row * N1 + j0, v, min(4, N1 - j0));
}

static inline bool zoom_step_ok(double z) { return isfinite(z) && z >= 0.0; }
static inline bool zoom_grid(long total, unsigned& blocks) {
  const long b = (total + 255) / 256;
  blocks = (unsigned)b;
  return b >= 1 && b <= 0x7fffffffL;
}

}  // namespace

extern "C" {
int arco_zoom_nearest2d(const void* src, int S, int n0, int n1, int N0, int N1, double z0, double z1, int elem_bytes, void* out,
                        void* stream) {
  ARCO_CHECK_ARG(src && out && S >= 1 && n0 >= 1 && n1 >= 1 && N0 >= 2 && N1 >= 2);
  ARCO_CHECK_ARG(elem_bytes == 4 || elem_bytes == 8);
  ARCO_CHECK_ARG(zoom_step_ok(z0) && zoom_step_ok(z1));
  const int vec = 16 / elem_bytes, runs = (N1 + vec - 1) / vec;
  const long total = (long)S * N0 * runs;
  unsigned blocks;
  ARCO_CHECK_ARG(zoom_grid(total, blocks));
  if (elem_bytes == 4)
    hipLaunchKernelGGL(zoom_nearest_kernel<uint32_t>, dim3(blocks), dim3(256), 0, as_stream(stream), (const uint32_t*)src, n0, n1, N0, N1,
                       runs, total, z0, z1, (uint32_t*)out);
  else
    hipLaunchKernelGGL(zoom_nearest_kernel<uint64_t>, dim3(blocks), dim3(256), 0, as_stream(stream), (const uint64_t*)src, n0, n1, N0, N1,
                       runs, total, z0, z1, (uint64_t*)out);
  return arco_launch_status();
}

extern "C++" {
template <typename T>
static int argmax_zoom_back_impl(const T* X, long ld, int C, int n, int P0, int P1, int N0, int N1, double z0, double z1, int64_t* out,
                                 void* stream) {
  ARCO_CHECK_ARG(X && out && C >= 1 && C <= ZOOM_MAXC && ld >= C && n >= 1 && P0 >= 1 && P1 >= 1 && N0 >= 2 && N1 >= 2);
  ARCO_CHECK_ARG(zoom_step_ok(z0) && zoom_step_ok(z1));
  const int runs = (N1 + 1) / 2;
  const long total = (long)n * N0 * runs;
  unsigned blocks;
  ARCO_CHECK_ARG(zoom_grid(total, blocks));
  hipLaunchKernelGGL(argmax_zoom_back_kernel<T>, dim3(blocks), dim3(256), 0, as_stream(stream), X, ld, C, P0, P1, N0, N1, runs, total, z0,
                     z1, reinterpret_cast<long*>(out));
  return arco_launch_status();
}
}  // extern "C++"
int arco_argmax_zoom_back2d(const float* X, long ld, int C, int n, int P0, int P1, int N0, int N1, double z0, double z1, int64_t* out,
                            void* stream) {
  return argmax_zoom_back_impl<float>(X, ld, C, n, P0, P1, N0, N1, z0, z1, out, stream);
}
// ... reading f16 logits rows (2-byte aligned at least): the class arco_argmax_zoom_back2d gives for the fp32 cast of the same rows
int arco_argmax_zoom_back2d_h(const void* X, long ld, int C, int n, int P0, int P1, int N0, int N1, double z0, double z1, int64_t* out,
                              void* stream) {
  ARCO_CHECK_ARG((reinterpret_cast<uintptr_t>(X) & 1) == 0);
  return argmax_zoom_back_impl<_Float16>(reinterpret_cast<const _Float16*>(X), ld, C, n, P0, P1, N0, N1, z0, z1, out, stream);
}

int arco_spline_prefilter2d(const float* src, int S, int n0, int n1, double z, double gain, double zn0, double zn1, int axes, double* out,
                            void* stream) {
  ARCO_CHECK_ARG(src && out && S >= 1 && n0 >= 2 && n1 >= 2 && axes >= 1 && axes <= 3);
  ARCO_CHECK_ARG(isfinite(z) && isfinite(gain) && isfinite(zn0) && isfinite(zn1));
  const long cols = (long)S * n1, rows = (long)S * n0;
  const long bc = (cols + 63) / 64, br = (rows + 63) / 64;
  ARCO_CHECK_ARG(bc <= 0x7fffffffL && br <= 0x7fffffffL);
  if (axes & 1)
    hipLaunchKernelGGL(spline_cols_kernel, dim3((unsigned)bc), dim3(64), 0, as_stream(stream), src, n0, n1, cols, SplinePole{z, gain, zn0}, out);
  if (axes & 2)
    hipLaunchKernelGGL(spline_rows_kernel, dim3((unsigned)br), dim3(64), 0, as_stream(stream), out, rows, n1, SplinePole{z, gain, zn1});
  return arco_launch_status();
}

int arco_zoom_cubic2d(const double* coef, int S, int n0, int n1, int N0, int N1, double z0, double z1, float* out, void* stream) {
  ARCO_CHECK_ARG(coef && out && S >= 1 && n0 >= 2 && n1 >= 2 && N0 >= 2 && N1 >= 2);
  ARCO_CHECK_ARG(n0 <= (1 << 30) && n1 <= (1 << 30));      // 2 (n - 1), the mirror period, is an int
  ARCO_CHECK_ARG(zoom_step_ok(z0) && zoom_step_ok(z1));
  const int runs = (N1 + 3) / 4;
  const long total = (long)S * N0 * runs;
  unsigned blocks;
  ARCO_CHECK_ARG(zoom_grid(total, blocks));
  hipLaunchKernelGGL(zoom_cubic_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), coef, n0, n1, N0, N1, runs, total, z0, z1, out);
  return arco_launch_status();
}
}  // extern "C"
