// The zoom(order=0) round trip of 2-D evaluation (test_2D.py:72-88; arco_amd/eval_surface.py predict_volume(zoom="gpu"),
// arco_amd/utils/zoom_gpu.py): every slice of a volume is resampled to the patch before the network and the arg-max map of the
// network is resampled back to the slice, both by scipy.ndimage.zoom(order=0, mode='constant').
//   zoom_nearest_kernel       [S][n0][n1] -> [S][N0][N1], 4- or 8-byte elements (nearest sampling moves bits: fp32 images, int64 labels)
//   argmax_zoom_back_kernel   logits rows [n * P0 * P1][ld] -> int64 labels [n][x][y]: the class of softmax_rows_kernel (glue.hip) of the
//                             ONE row each output pixel samples; rows no output pixel samples are never read
// Pure streams: a thread writes 16 bytes of consecutive outputs of the fastest axis (one store where the address allows it, scalar stores
// otherwise and at the ragged end of a row), no LDS, no atomics.
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
__device__ __forceinline__ long row_class(const float* __restrict__ x, int C) {
#pragma clang fp contract(fast)
  float v[ZOOM_MAXC];
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < ZOOM_MAXC; ++c) if (c < C) { v[c] = x[c]; mx = fmaxf(mx, v[c]); }
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
__global__ __launch_bounds__(256) void argmax_zoom_back_kernel(const float* __restrict__ X, long ld, int C, int P0, int P1, int N0, int N1,
                                                               int runs, long total, double z0, double z1, long* __restrict__ out) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= total) return;
  const long row = q / runs;
  const int j0 = (int)(q - row * runs) * 2, i = (int)(row % N0);
  const long s = row / N0;
  long v[2] = {0, 0};
  int su;
  if (zoom_index(i, z0, P0, su)) {
    const float* line = X + (s * P0 + su) * P1 * ld;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      int sv;
      if (j0 + e < N1 && zoom_index(j0 + e, z1, P1, sv)) v[e] = row_class(line + sv * ld, C);
    }
  }
  store_run<long, 2>(out + row * N1 + j0, v, min(2, N1 - j0));
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

int arco_argmax_zoom_back2d(const float* X, long ld, int C, int n, int P0, int P1, int N0, int N1, double z0, double z1, int64_t* out,
                            void* stream) {
  ARCO_CHECK_ARG(X && out && C >= 1 && C <= ZOOM_MAXC && ld >= C && n >= 1 && P0 >= 1 && P1 >= 1 && N0 >= 2 && N1 >= 2);
  ARCO_CHECK_ARG(zoom_step_ok(z0) && zoom_step_ok(z1));
  const int runs = (N1 + 1) / 2;
  const long total = (long)n * N0 * runs;
  unsigned blocks;
  ARCO_CHECK_ARG(zoom_grid(total, blocks));
  hipLaunchKernelGGL(argmax_zoom_back_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), X, ld, C, P0, P1, N0, N1, runs, total, z0, z1,
                     reinterpret_cast<long*>(out));
  return arco_launch_status();
}
}  // extern "C"
