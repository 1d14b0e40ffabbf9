// Data ingest from a GPU-resident dataset (trainers' --gpu_ingest 1; arco_amd/dataloaders/gpu_ingest.py): one launch turns a batch of
// per-sample transform descriptors into the batch the host transforms would have produced, bit for bit.
//   2-D (dataloaders/dataset.py RandomGenerator): zoom(order=0) to the patch, then one of no-op / rot90+flip / rotate(order=0) / centre crop.
//   3-D (dataloaders/la_heart.py): RandomRotFlip -> RandomCrop (symmetric zero pad, random offsets) -> ToTensor.
// Every transform is nearest-neighbour or an index map, so each output element walks the chain BACKWARDS to one stored element (or
// the constant 0).  Pure streams: a thread writes four consecutive outputs of the fastest axis (one 16-byte image store, two 16-byte
// label stores), no LDS, no atomics.
//
// The coordinate arithmetic is scipy.ndimage's (ni_interpolation.c, NI_ZoomShift / NI_GeometricTransform with order 0, mode
// 'constant'), in float64 with every product and sum rounded separately: a contracted multiply-add moves a coordinate by an ulp and
// with it a tie of floor(cc + 0.5) or the `cc > n - 1` test that zeroes a whole last row.  Contraction is therefore off for the file,
// and the products and sums are written as plain operators below it: the __dmul_rn / __dadd_rn of the HIP headers are defined BEFORE
// this pragma, carry the `contract` flag, and fuse once inlined (seen in the ISA as v_fma_f64).
#pragma clang fp contract(off)
#include "common.h"

namespace {

#define INGEST_SLICE_DESC 16     // doubles per 2-D sample, see SliceDesc
#define INGEST_VOLUME_DESC 8     // int64 per 3-D sample: case, k, axis, s0, s1, s2, 0, 0
#define INGEST_TABLE 4           // int64 per case: offset (elements), n0, n1, n2 (1 for slices)

// One 2-D sample (a row of 16 doubles; the integers are exact in float64):
//   [0] case  [1] op (0 none, 1 rot90 + flip, 2 rotate, 3 crop)  [2] Z0 [3] Z1 zoomed shape  [4] z0 [5] z1 = (n_in - 1) / (Z - 1)
//   [6] a [7] b : op 1: k, axis   op 3: shift of the crop window in the zoomed image, rows / columns (may be negative: zero pad)
//   [8..11] m00 m01 m10 m11  [12] off0 [13] off1 : op 2, the matrix and offset scipy.ndimage.rotate hands to affine_transform
struct SliceDesc {
  long cs; int op, Z0, Z1, a, b;
  double z0, z1, m00, m01, m10, m11, off0, off1;
};

__device__ __forceinline__ SliceDesc load_slice_desc(const double* __restrict__ d) {
  SliceDesc s;
  s.cs = (long)d[0]; s.op = (int)d[1]; s.Z0 = (int)d[2]; s.Z1 = (int)d[3]; s.z0 = d[4]; s.z1 = d[5]; s.a = (int)d[6]; s.b = (int)d[7];
  s.m00 = d[8]; s.m01 = d[9]; s.m10 = d[10]; s.m11 = d[11]; s.off0 = d[12]; s.off1 = d[13];
  return s;
}

__device__ __forceinline__ double dmul(double a, double b) { return a * b; }
__device__ __forceinline__ double dadd(double a, double b) { return a + b; }

// order-0 sample position for coordinate cc on an axis of n points, mode 'constant': outside [0, n - 1] the constant, else floor(cc + 0.5)
__device__ __forceinline__ bool nearest(double cc, int n, int& idx) {
  if (!(cc >= 0.0 && cc <= (double)(n - 1))) return false;
  idx = (int)floor(dadd(cc, 0.5));
  return true;
}

// inverse of flip(rot90(a, k), axis) for an output of shape (R0, R1) and a source of shape (N0, N1): output (r, c) -> source (u, v)
__device__ __forceinline__ void unrotflip(int k, int axis, int R0, int R1, int N0, int N1, int r, int c, int& u, int& v) {
  if (axis == 0) r = R0 - 1 - r; else c = R1 - 1 - c;
  switch (k & 3) {
    case 0: u = r; v = c; break;
    case 1: u = c; v = N1 - 1 - r; break;
    case 2: u = N0 - 1 - r; v = N1 - 1 - c; break;
    default: u = N0 - 1 - c; v = r; break;
  }
}

// stored element of output pixel (i, j) of a 2-D sample, or -1 for the constant 0
__device__ __forceinline__ long slice_source(const SliceDesc& s, int n0, int n1, int H, int W, int i, int j) {
  int u = i, v = j;
  if (s.op == 1) {
    unrotflip(s.a, s.b, H, W, s.Z0, s.Z1, i, j, u, v);
  } else if (s.op == 2) {
    const double c0 = dadd(dadd(s.off0, dmul((double)i, s.m00)), dmul((double)j, s.m01));
    const double c1 = dadd(dadd(s.off1, dmul((double)i, s.m10)), dmul((double)j, s.m11));
    if (!nearest(c0, s.Z0, u) || !nearest(c1, s.Z1, v)) return -1;
  } else if (s.op == 3) {
    u = i + s.a; v = j + s.b;
  }
  if (u < 0 || u >= s.Z0 || v < 0 || v >= s.Z1) return -1;     // the crop's zero pad (and the guard of a descriptor that does not fit)
  int su, sv;
  if (!nearest(dmul((double)u, s.z0), n0, su) || !nearest(dmul((double)v, s.z1), n1, sv)) return -1;
  return (long)su * n1 + sv;
}

__device__ __forceinline__ void store_labels(long* __restrict__ p, const long (&l)[4]) {
  typedef long l64x2 __attribute__((ext_vector_type(2)));
  *reinterpret_cast<l64x2*>(p) = l64x2{l[0], l[1]};
  *reinterpret_cast<l64x2*>(p + 2) = l64x2{l[2], l[3]};
}

__global__ __launch_bounds__(256) void ingest_slices_kernel(const float* __restrict__ bank_img, const unsigned char* __restrict__ bank_lab,
                                                            long bank_elems, const long* __restrict__ table, long n_cases,
                                                            const double* __restrict__ desc, int H, int W,
                                                            float* __restrict__ out_img, long* __restrict__ out_lab) {
  const int W4 = W >> 2;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long)H * W4) return;
  const int b = blockIdx.y, i = (int)(q / W4), j0 = (int)(q % W4) * 4;
  const SliceDesc s = load_slice_desc(desc + (long)b * INGEST_SLICE_DESC);
  long off = 0; int n0 = 0, n1 = 0;
  bool live = s.cs >= 0 && s.cs < n_cases && s.Z0 > 0 && s.Z1 > 0;
  if (live) {
    const long* t = table + s.cs * INGEST_TABLE;
    off = t[0]; n0 = (int)t[1]; n1 = (int)t[2];
    live = off >= 0 && n0 > 0 && n1 > 0 && off + (long)n0 * n1 <= bank_elems;
  }
  f32x4 px = {0.f, 0.f, 0.f, 0.f};
  long lb[4] = {0, 0, 0, 0};
  if (live) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long src = slice_source(s, n0, n1, H, W, i, j0 + e);
      if (src >= 0) { px[e] = bank_img[off + src]; lb[e] = (long)bank_lab[off + src]; }
    }
  }
  const long o = ((long)b * H + i) * W + j0;
  st4f(out_img + o, px);
  if (out_lab) store_labels(out_lab + o, lb);
}

__global__ __launch_bounds__(256) void ingest_volumes_kernel(const float* __restrict__ bank_img, const unsigned char* __restrict__ bank_lab,
                                                             long bank_elems, const long* __restrict__ table, long n_cases,
                                                             const long* __restrict__ desc, int X, int Y, int Z,
                                                             float* __restrict__ out_img, long* __restrict__ out_lab) {
  const int Z4 = Z >> 2;
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long)X * Y * Z4) return;
  const int b = blockIdx.y, z0 = (int)(q % Z4) * 4, y = (int)((q / Z4) % Y), x = (int)(q / ((long)Z4 * Y));
  const long* d = desc + (long)b * INGEST_VOLUME_DESC;
  const long cs = d[0];
  const int k = (int)d[1], axis = (int)d[2];
  f32x4 px = {0.f, 0.f, 0.f, 0.f};
  long lb[4] = {0, 0, 0, 0};
  if (cs >= 0 && cs < n_cases) {
    const long* t = table + cs * INGEST_TABLE;
    const long off = t[0];
    const int n0 = (int)t[1], n1 = (int)t[2], n2 = (int)t[3];
    const int R0 = (k & 1) ? n1 : n0, R1 = (k & 1) ? n0 : n1;                 // shape after rot90 in the first two axes
    // position in the rotated, flipped, unpadded volume: crop offset minus pad (negative or past the end: the zero pad)
    const long r = (long)x + d[3], c = (long)y + d[4], zs = (long)z0 + d[5];
    if (off >= 0 && n0 > 0 && n1 > 0 && n2 > 0 && off + (long)n0 * n1 * n2 <= bank_elems && r >= 0 && r < R0 && c >= 0 && c < R1) {
      int u, v;
      unrotflip(k, axis, R0, R1, n0, n1, (int)r, (int)c, u, v);
      const long row = off + ((long)u * n1 + v) * n2;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long zz = zs + e;
        if (zz >= 0 && zz < n2) { px[e] = bank_img[row + zz]; lb[e] = (long)bank_lab[row + zz]; }
      }
    }
  }
  const long o = (((long)b * X + x) * Y + y) * Z + z0;
  st4f(out_img + o, px);
  if (out_lab) store_labels(out_lab + o, lb);
}

static inline bool host_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {
/* bank_img / bank_lab: the packed cases (fp32 / uint8, bank_elems elements each); table: [n_cases][4] int64 {offset, n0, n1, n2};
   desc: [B][16] float64 on the device (SliceDesc above); out_img [B,1,H,W] fp32, out_lab [B,H,W] int64 or null (labels not wanted).
   W % 4 == 0; the outputs 16-byte aligned. */
int arco_ingest_slices(const float* bank_img, const unsigned char* bank_lab, long bank_elems, const long* table, long n_cases,
                       const double* desc, int B, int H, int W, float* out_img, long* out_lab, void* stream) {
  ARCO_CHECK_ARG(bank_img && bank_lab && table && desc && out_img && bank_elems > 0 && n_cases > 0);
  ARCO_CHECK_ARG(B >= 1 && B <= 65535 && H >= 2 && W >= 4 && W % 4 == 0);
  ARCO_CHECK_ARG(host_al16(out_img) && host_al16(out_lab));
  const long quads = (long)H * (W / 4);
  ARCO_CHECK_ARG((quads + 255) / 256 <= 0x7fffffffL);
  hipLaunchKernelGGL(ingest_slices_kernel, dim3((unsigned)((quads + 255) / 256), B), dim3(256), 0, as_stream(stream), bank_img, bank_lab,
                     bank_elems, table, n_cases, desc, H, W, out_img, out_lab);
  return arco_launch_status();
}
/* desc: [B][8] int64 {case, k, axis, s0, s1, s2, 0, 0}: k quarter turns in the first two axes, flip along axis (0 / 1), s = crop
   offset minus pad per axis; out_img [B,1,X,Y,Z] fp32, out_lab [B,X,Y,Z] int64 or null.  Z % 4 == 0. */
int arco_ingest_volumes(const float* bank_img, const unsigned char* bank_lab, long bank_elems, const long* table, long n_cases,
                        const long* desc, int B, int X, int Y, int Z, float* out_img, long* out_lab, void* stream) {
  ARCO_CHECK_ARG(bank_img && bank_lab && table && desc && out_img && bank_elems > 0 && n_cases > 0);
  ARCO_CHECK_ARG(B >= 1 && B <= 65535 && X >= 1 && Y >= 1 && Z >= 4 && Z % 4 == 0);
  ARCO_CHECK_ARG(host_al16(out_img) && host_al16(out_lab));
  const long quads = (long)X * Y * (Z / 4);
  ARCO_CHECK_ARG((quads + 255) / 256 <= 0x7fffffffL);
  hipLaunchKernelGGL(ingest_volumes_kernel, dim3((unsigned)((quads + 255) / 256), B), dim3(256), 0, as_stream(stream), bank_img, bank_lab,
                     bank_elems, table, n_cases, desc, X, Y, Z, out_img, out_lab);
  return arco_launch_status();
}
}  // extern "C"
