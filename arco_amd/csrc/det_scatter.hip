// Order-independent row scatter: the adjoint of the row-sparse head's gathers with a bit-reproducible result.
//
// The backward of `F.interpolate(...)[rows]` / `x[rows]` (model_3D.py:46-58 evaluated at the sampled voxels, arco_amd/head.py) adds
// several source rows into one destination row: neighbouring anchors share low-resolution corners, anchors are drawn with
// replacement (loss_helper_3d.py:455-457).  With fp32 atomics the sum depends on the order in which the waves arrive: one ulp.
// On fp32 activations that is where it stays (as it does in torch's own upsample backward, which the reference runs); with f16
// activation STORAGE (--act_dtype f16) the FeatureExtractor's data gradient is rounded to f16 on its way into the V-Net's
// backward, the ulp decides a rounding now and then, and every later rounding amplifies the difference: two executions of the
// same LiTS-shaped step differed by 4.7e-5 of the largest gradient element (tools/debug/repro3d.py, profiles/r05_notes.md
// section 7).  Here every contribution is converted to a fixed-point integer of a common scale - 2^44 units for the largest
// |source element| of the launch, found by an atomicMax over bit patterns, itself order-independent - and accumulated with 64-bit
// integer atomics: integer addition is associative, the sum does not depend on the order, and one int64 -> fp32 conversion
// rounds it once.  Resolution 2^-44 of the largest element (fp32's own: 2^-24 of EACH element; a sum's error in fp32 is set by
// its largest terms), headroom 2^18 colliding contributions.
//
// The accumulator is a persistent int64 buffer, zero by invariant: finish converts the touched rows into the fp32 destination
// (overwriting: the destination rows hold nothing else), clear re-zeroes them.
#include "interp.h"
#include "split_bf16.h"

#define DET_BITS 44

// maxbits[0] = max over the [n, C] matrix of (bits(x) & 0x7fffffff): >= 0x7f800000 when any element is inf / nan
__global__ __launch_bounds__(256) void det_absmax_kernel(const float* __restrict__ X, long ld, int C, long n, unsigned* __restrict__ out) {
  unsigned m = 0;
  const long tot = n * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < tot; i += (long)gridDim.x * 256) {
    const long r = i / C; const int c = (int)(i - r * C);
    const unsigned b = __float_as_uint(X[r * ld + c]) & 0x7fffffffu;
    m = b > m ? b : m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned t = __shfl_xor(m, o, 64); m = t > m ? t : m; }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// an fp32 product the SLP vectoriser cannot pair into v_pk_mul_f32: left to itself it emitted the cross-select form of the gfx950
// erratum for the corner weights below (tests/test_isa_lint.py caught it)
__device__ __forceinline__ float mul_np(float a, float b) { float r; asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

// largest element < 2^(e - 126)  ->  scaled by 2^sh it stays below 2^DET_BITS
__device__ __forceinline__ int det_shift(unsigned maxbits) { return DET_BITS + 126 - (int)(maxbits >> 23); }

// acc[r(e)][c] += fix(w[e] * src[e / div][c]),  r(e) = list ? list[idx[e]] : idx[e]
__global__ __launch_bounds__(256) void det_scatter_rows_kernel(const float* __restrict__ src, long lds_, int C, int div,
                                                              const int32_t* __restrict__ list, const int64_t* __restrict__ idx,
                                                              const float* __restrict__ w, long n_e, long long* __restrict__ acc, long lda,
                                                              const unsigned* __restrict__ maxbits) {
  const int lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= n_e) return;
  const unsigned mb = maxbits[0];
  if (mb >= 0x7f800000u || mb == 0) return;          // non-finite source: finish writes nan; all-zero source: nothing to add
  const int sh = det_shift(mb);
  long r = idx[e];
  if (list) r = list[r];
  const float wt = w ? w[e] : 1.f;
  const float* s = src + (e / div) * lds_;
  unsigned long long* a = reinterpret_cast<unsigned long long*>(acc + r * lda);
  for (int c = lane; c < C; c += 64) {
    const long long q = __float2ll_rn(ldexpf(wt * s[c], sh));
    if (q) atomicAdd(a + c, (unsigned long long)q);
  }
}

// dst[r(e)][c] = alpha * float(acc[r(e)][c]) * 2^-sh   (rows listed more than once are written more than once, with the same bits)
__global__ __launch_bounds__(256) void det_finish_rows_kernel(const int32_t* __restrict__ list, const int64_t* __restrict__ idx, long n_e,
                                                             const long long* __restrict__ acc, long lda, int C,
                                                             const unsigned* __restrict__ maxbits, float alpha,
                                                             float* __restrict__ dst, long ldd) {
  const int lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= n_e) return;
  const unsigned mb = maxbits[0];
  long r = idx[e];
  if (list) r = list[r];
  float* d = dst + r * ldd;
  if (mb >= 0x7f800000u) {
    for (int c = lane; c < C; c += 64) d[c] = __uint_as_float(0x7fc00000u);
    return;
  }
  if (mb == 0) return;
  const int sh = det_shift(mb);
  const long long* a = acc + r * lda;
  for (int c = lane; c < C; c += 64) d[c] = alpha * ldexpf(__ll2float_rn(a[c]), -sh);
}

__global__ __launch_bounds__(256) void det_clear_rows_kernel(const int32_t* __restrict__ list, const int64_t* __restrict__ idx, long n_e,
                                                            long long* __restrict__ acc, long lda, int C) {
  const int lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= n_e) return;
  long r = idx[e];
  if (list) r = list[r];
  long long* a = acc + r * lda;
  for (int c = lane; c < C; c += 64) a[c] = 0;
}

// The eight low-resolution corners of every sampled output voxel of an align_corners trilinear resize [Di,Hi,Wi] -> [Do,Ho,Wo]:
// idx8[8 j + k] = row of corner k in the channels-last low-resolution tensor, w8[8 j + k] = its interpolation weight
// (the same index / weight arithmetic as the gather: igemm_args.h ac_src; corner order z, y, x with x fastest)
__global__ __launch_bounds__(256) void corner_rows3d_kernel(const int64_t* __restrict__ pix, long n, int Di, int Hi, int Wi, int Do, int Ho,
                                                           int Wo, int64_t* __restrict__ idx8, float* __restrict__ w8) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const long p = pix[j];
  const long vol = (long)Do * Ho * Wo;
  const long img = p / vol; long rem = p - img * vol;
  const int zo = (int)(rem / ((long)Ho * Wo)); rem -= (long)zo * Ho * Wo;
  const int yo = (int)(rem / Wo), xo = (int)(rem - (long)yo * Wo);
  const float sd = Do > 1 ? (float)(Di - 1) / (float)(Do - 1) : 0.f, sh = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f,
              sw = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
  int zz[2], yy[2], xx[2]; float lz, ly, lx;
  ac_src(zo, sd, Di, zz[0], zz[1], lz); ac_src(yo, sh, Hi, yy[0], yy[1], ly); ac_src(xo, sw, Wi, xx[0], xx[1], lx);
  const float wz[2] = {1.f - lz, lz}, wy[2] = {1.f - ly, ly}, wx[2] = {1.f - lx, lx};
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const int k = a * 4 + b * 2 + d;
        idx8[8 * j + k] = ((img * Di + zz[a]) * (long)Hi + yy[b]) * Wi + xx[d];
        w8[8 * j + k] = mul_np(mul_np(wz[a], wy[b]), wx[d]);
      }
}

// flag[r] = 1 when row r of X [M, C] holds any element that is not +-0 (nan and inf count): the gradient of a dense per-pixel layer
// whose loss reads a few sampled rows is zero everywhere else, and the 1x1 convolutions' backward (ops.ConvFn) then runs on the
// flagged rows only.  One wave per 4 rows x 64 lanes of 16-byte loads; reads X once.
__global__ __launch_bounds__(256) void row_nonzero_kernel(const float* __restrict__ X, long ld, int C, long M, unsigned char* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const long r = ((long)blockIdx.x * 4 + (threadIdx.x >> 6));
  if (r >= M) return;
  const float* x = X + r * ld;
  unsigned any = 0;
  const int C4 = C & ~3;
  for (int c = lane * 4; c < C4; c += 256) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(x + c);
    any |= (v[0] | v[1] | v[2] | v[3]) & 0x7fffffffu;
  }
  for (int c = C4 + lane; c < C; c += 64) any |= __float_as_uint(x[c]) & 0x7fffffffu;
  const unsigned long long b = __ballot(any != 0);
  if (lane == 0) flag[r] = b ? 1 : 0;
}
// dst[idx[j]][0..C) = src[j][0..C)   (idx without repetitions: plain stores)
__global__ __launch_bounds__(256) void put_rows_kernel(const float* __restrict__ src, long lds_, int C, const int64_t* __restrict__ idx, long n,
                                                      float* __restrict__ dst, long ldd) {
  const int lane = threadIdx.x & 63;
  const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;
  const float* s = src + j * lds_;
  float* d = dst + idx[j] * ldd;
  for (int c = lane * 4; c < (C & ~3); c += 256) *reinterpret_cast<f32x4*>(d + c) = *reinterpret_cast<const f32x4*>(s + c);
  for (int c = (C & ~3) + lane; c < C; c += 64) d[c] = s[c];
}

// 2-D counterpart (bilinear, align_corners: the adjoint of gather_upcat_rows, elementwise.hip): four corners y, x with x fastest
__global__ __launch_bounds__(256) void corner_rows2d_kernel(const int64_t* __restrict__ pix, long n, int Hi, int Wi, int Ho, int Wo,
                                                           int64_t* __restrict__ idx4, float* __restrict__ w4) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const long p = pix[j];
  const long img = p / ((long)Ho * Wo); const int rem = (int)(p - img * (long)Ho * Wo);
  const int yo = rem / Wo, xo = rem - yo * Wo;
  const float sh = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f, sw = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
  int yy[2], xx[2]; float ly, lx;
  ac_src(yo, sh, Hi, yy[0], yy[1], ly); ac_src(xo, sw, Wi, xx[0], xx[1], lx);
  const float wy[2] = {1.f - ly, ly}, wx[2] = {1.f - lx, lx};
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      idx4[4 * j + b * 2 + d] = (img * Hi + yy[b]) * (long)Wi + xx[d];
      w4[4 * j + b * 2 + d] = mul_np(wy[b], wx[d]);
    }
}

extern "C" {

int arco_det_absmax(const float* X, long ld, int C, long n, unsigned* maxbits, void* stream) {
  ARCO_CHECK_ARG(X && maxbits && C > 0 && n >= 0);
  if (hipMemsetAsync(maxbits, 0, sizeof(unsigned), as_stream(stream)) != hipSuccess) return ARCO_ERR_LAUNCH;
  if (n == 0) return ARCO_OK;
  long blocks = (n * C + 255) / 256; if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(det_absmax_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), X, ld, C, n, maxbits);
  return arco_launch_status();
}

int arco_det_scatter_rows(const float* src, long ld_src, int C, int div, const int32_t* list, const int64_t* idx, const float* w,
                          long n_e, long long* acc, long ld_acc, const unsigned* maxbits, void* stream) {
  ARCO_CHECK_ARG(src && idx && acc && maxbits && C > 0 && div >= 1 && n_e >= 0 && (reinterpret_cast<uintptr_t>(acc) & 7) == 0);
  if (n_e == 0) return ARCO_OK;
  hipLaunchKernelGGL(det_scatter_rows_kernel, dim3((unsigned)((n_e + 3) / 4)), dim3(256), 0, as_stream(stream), src, ld_src, C, div, list,
                     idx, w, n_e, acc, ld_acc, maxbits);
  return arco_launch_status();
}

int arco_det_finish_rows(const int32_t* list, const int64_t* idx, long n_e, const long long* acc, long ld_acc, int C,
                         const unsigned* maxbits, float alpha, float* dst, long ld_dst, void* stream) {
  ARCO_CHECK_ARG(idx && acc && maxbits && dst && C > 0 && n_e >= 0);
  if (n_e == 0) return ARCO_OK;
  hipLaunchKernelGGL(det_finish_rows_kernel, dim3((unsigned)((n_e + 3) / 4)), dim3(256), 0, as_stream(stream), list, idx, n_e, acc, ld_acc,
                     C, maxbits, alpha, dst, ld_dst);
  return arco_launch_status();
}

int arco_det_clear_rows(const int32_t* list, const int64_t* idx, long n_e, long long* acc, long ld_acc, int C, void* stream) {
  ARCO_CHECK_ARG(idx && acc && C > 0 && n_e >= 0);
  if (n_e == 0) return ARCO_OK;
  hipLaunchKernelGGL(det_clear_rows_kernel, dim3((unsigned)((n_e + 3) / 4)), dim3(256), 0, as_stream(stream), list, idx, n_e, acc, ld_acc, C);
  return arco_launch_status();
}

int arco_corner_rows3d(const int64_t* pix, long n, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int64_t* idx8, float* w8,
                       void* stream) {
  ARCO_CHECK_ARG(pix && idx8 && w8 && Di > 0 && Hi > 0 && Wi > 0 && Do > 0 && Ho > 0 && Wo > 0 && n >= 0);
  if (n == 0) return ARCO_OK;
  hipLaunchKernelGGL(corner_rows3d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), pix, n, Di, Hi, Wi, Do, Ho, Wo,
                     idx8, w8);
  return arco_launch_status();
}

int arco_corner_rows2d(const int64_t* pix, long n, int Hi, int Wi, int Ho, int Wo, int64_t* idx4, float* w4, void* stream) {
  ARCO_CHECK_ARG(pix && idx4 && w4 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && n >= 0);
  if (n == 0) return ARCO_OK;
  hipLaunchKernelGGL(corner_rows2d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), pix, n, Hi, Wi, Ho, Wo, idx4, w4);
  return arco_launch_status();
}

int arco_row_nonzero(const float* X, long ld, int C, long M, unsigned char* flag, void* stream) {
  ARCO_CHECK_ARG(X && flag && C > 0 && M >= 0 && (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0);
  if (M == 0) return ARCO_OK;
  hipLaunchKernelGGL(row_nonzero_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, as_stream(stream), X, ld, C, M, flag);
  return arco_launch_status();
}

int arco_put_rows(const float* src, long ld_src, int C, const int64_t* idx, long n, float* dst, long ld_dst, void* stream) {
  ARCO_CHECK_ARG(src && idx && dst && C > 0 && n >= 0 && (ld_src & 3) == 0 && (ld_dst & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(dst) & 15) == 0);
  if (n == 0) return ARCO_OK;
  hipLaunchKernelGGL(put_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream), src, ld_src, C, idx, n, dst, ld_dst);
  return arco_launch_status();
}

}  // extern "C"
