// f16 ACTIVATION STORAGE for the 2-D path (train_arco_2d --act_dtype f16): the U-Net operators of unetWithArgs.py that conv_h.hip
// and the *_h forms of elementwise.hip do not cover.  Conventions as in conv_h.hip: f16 in HBM, fp32 arithmetic, one rounding per
// stored value, channels-last rows, fp32 BatchNorm statistics of the ROUNDED outputs.
//
//   himage_conv_kernel    the first layer: 3x3 convolution of the fp32 IMAGE (1 - 4 channels) to 16 channels, stored as f16 - this
//                         layer opens the f16 region (conv3x3_image_kernel's streaming form: 9 * Cin multiply-adds per value).
//   himage_wgrad_kernel   its weight gradient dW[co][ci][tap] = sum_pix dZ[pix][co] X[pix + tap][ci] from the f16 dZ and the fp32
//                         image: a thread owns one (co, tap, ci) element (up to 576 of them) over a 16 x 16 tile staged in LDS,
//                         one slab per persistent workgroup -> wgrad_reduce (fixed order, deterministic).
//   hmaxpool2_*           nn.MaxPool2d(2) forward / backward (+ the skip connection's gradient) on f16: a maximum and a routed
//                         value need no rounding; the sum with the skip gradient is formed in fp32 and rounded once.
//   hbilinear_*           align_corners bilinear resize (the x2 upsample written behind the skip in the concat buffer) and its
//                         adjoint: bilinear_fwd_kernel's / bilinear_bwd_kernel's index math and summation order in fp32, rounded
//                         once on store.
// The VALU kernels move 8 channels (16 bytes) per lane.
#include <initializer_list>
#include "sp_util.h"
#include "interp.h"
#include "wgrad.h"

typedef _Float16 uh8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

static inline int uh_grid(long work) {
  long g = (work + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}
__device__ __forceinline__ f32x8 ld8h(const _Float16* p) { return __builtin_convertvector(*reinterpret_cast<const uh8*>(p), f32x8); }
__device__ __forceinline__ void st8h(_Float16* p, f32x8 v) { *reinterpret_cast<uh8*>(p) = __builtin_convertvector(v, uh8); }

// ---------------------------------------------------------------------------------------------------------------------
// first layer, forward
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void himage_conv_kernel(const float* __restrict__ X, long ldx, int K, const float* __restrict__ Wp,
                                                         int N, int Npad, int Kpad, const float* __restrict__ bias,
                                                         _Float16* __restrict__ C, long ldc, int NB, int H, int W,
                                                         float* __restrict__ stat_sum, float* __restrict__ stat_sq, int n_grp) {
  constexpr int TH = 16, TW = 16, HW_ = TW + 2, NP = (TH + 2) * HW_;
  __shared__ float Xs[4][NP];            // [k][halo pixel]
  __shared__ __attribute__((aligned(16))) float Ws[9 * 4 * 16];   // [tap][k][n]
  __shared__ float red[2][4][16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int pl = tid >> 2, qd = tid & 3;                         // pixel of the tile (0..63), channel quad
  for (int u = tid; u < 9 * 4 * 16; u += 256) {
    const int n = u & 15, k = (u >> 4) & 3, tap = u >> 6;
    Ws[u] = (k < K && n < Npad) ? Wp[((long)tap * Npad + n) * Kpad + k] : 0.f;
  }
  f32x4 bias4 = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 4; ++e) if (bias && 4 * qd + e < N) bias4[e] = bias[4 * qd + e];
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const long n_tiles = (long)NB * tiles_y * tiles_x;
  f32x4 s1 = {0, 0, 0, 0}, s2 = {0, 0, 0, 0};
  const int bpg = gridDim.x / n_grp;                             // one BN group per workgroup
  const long tpg = n_tiles / n_grp, t_end = (blockIdx.x / bpg + 1) * tpg;
  for (long t = (blockIdx.x / bpg) * tpg + blockIdx.x % bpg; t < t_end; t += bpg) {
    const int tx = t % tiles_x; const long r = t / tiles_x; const int ty = r % tiles_y; const int nb = r / tiles_y;
    __syncthreads();
    for (int u = tid; u < NP * K; u += 256) {
      const int k = u % K, hp = u / K, hy = hp / HW_, hx = hp % HW_;
      const int gy = ty * TH + hy - 1, gx = tx * TW + hx - 1;
      Xs[k][hp] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? X[(((long)nb * H + gy) * W + gx) * ldx + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TH * TW / 64; ++i) {                     // 4 pixels per lane: rows py, py + 4, ...
      const int p = pl + 64 * i, py = p / TW, px = p % TW;
      f32x4 acc = bias4;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int hp = (py + tap / 3) * HW_ + px + tap % 3;
        for (int k = 0; k < K; ++k) {
          const float x = Xs[k][hp];
          const f32x4 wv = *reinterpret_cast<const f32x4*>(&Ws[(tap * 4 + k) * 16 + 4 * qd]);
          acc += wv * x;
        }
      }
      const int gy = ty * TH + py, gx = tx * TW + px;
      if (gy < H && gx < W && 4 * qd < N) {
        const long pix = ((long)nb * H + gy) * W + gx;
        const f16x4 hv = to_f16x4(acc);
        *reinterpret_cast<f16x4*>(C + pix * ldc + 4 * qd) = hv;
        acc = __builtin_convertvector(hv, f32x4);                // statistics of the rounded values
        s1 += acc; s2 += acc * acc;
      }
    }
  }
  if (stat_sum) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v1 = s1[e], v2 = s2[e];
#pragma unroll
      for (int o = 4; o < 64; o <<= 1) { v1 += __shfl_xor(v1, o, 64); v2 += __shfl_xor(v2, o, 64); }
      if (lane < 4) { red[0][w][4 * lane + e] = v1; red[1][w][4 * lane + e] = v2; }
    }
    __syncthreads();
    if (tid < 16 && tid < N) {
      stat_sum[(long)tid * gridDim.x + blockIdx.x] = (red[0][0][tid] + red[0][1][tid]) + (red[0][2][tid] + red[0][3][tid]);
      stat_sq[(long)tid * gridDim.x + blockIdx.x] = (red[1][0][tid] + red[1][1][tid]) + (red[1][2][tid] + red[1][3][tid]);
    }
  }
}

static long himage_blocks(int NB, int H, int W, int n_grp) {
  const long n_tiles = (long)NB * ((H + 15) / 16) * ((W + 15) / 16);
  long bpg = 1024 / n_grp; if (bpg > n_tiles / n_grp) bpg = n_tiles / n_grp; if (bpg < 1) bpg = 1;
  return bpg * n_grp;
}

// ---------------------------------------------------------------------------------------------------------------------
// first layer, weight gradient
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void himage_wgrad_kernel(const _Float16* __restrict__ dZ, long ldz, const float* __restrict__ X,
                                                          long ldx, int K, int NB, int H, int W, float* __restrict__ partial) {
  constexpr int TH = 16, TW = 16, HW_ = TW + 2, NP = (TH + 2) * HW_;
  __shared__ float Xs[4][NP];
  __shared__ __attribute__((aligned(32))) float Zs[256 * 16];     // dZ tile [pixel][co], zero outside the image
  const int tid = threadIdx.x;
  const int n_out = 144 * K;                                      // element o = co + 16 * (tap + 9 * ci)
  int zo[3], xo[3], ck[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int o = tid + 256 * j, oo = o < n_out ? o : 0;
    const int co = oo & 15, tc = oo >> 4, tap = tc % 9, ci = tc / 9;
    zo[j] = co; ck[j] = ci; xo[j] = (tap / 3) * HW_ + tap % 3;
  }
  float acc[3] = {0.f, 0.f, 0.f};
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const long n_tiles = (long)NB * tiles_y * tiles_x;
  for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int tx = t % tiles_x; const long r = t / tiles_x; const int ty = r % tiles_y; const int nb = r / tiles_y;
    __syncthreads();
    for (int u = tid; u < NP * K; u += 256) {
      const int k = u % K, hp = u / K, hy = hp / HW_, hx = hp % HW_;
      const int gy = ty * TH + hy - 1, gx = tx * TW + hx - 1;
      Xs[k][hp] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? X[(((long)nb * H + gy) * W + gx) * ldx + k] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int u = tid + 256 * i, p = u >> 1, q = u & 1;
      const int gy = ty * TH + (p >> 4), gx = tx * TW + (p & 15);
      f32x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (gy < H && gx < W) v = ld8h(dZ + (((long)nb * H + gy) * W + gx) * ldz + 8 * q);
      *reinterpret_cast<f32x8*>(&Zs[p * 16 + 8 * q]) = v;
    }
    __syncthreads();
    for (int p = 0; p < 256; ++p) {
      const int hp = (p >> 4) * HW_ + (p & 15);
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] = __builtin_fmaf(Zs[p * 16 + zo[j]], Xs[ck[j]][hp + xo[j]], acc[j]);
    }
  }
  // slab [tap][16][16] of this workgroup (layout of the generic kernels; ci >= K is never read)
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int o = tid + 256 * j;
    if (o < n_out) {
      const int co = o & 15, tc = o >> 4, tap = tc % 9, ci = tc / 9;
      partial[(((long)blockIdx.x * 9 + tap) * 16 + co) * 16 + ci] = acc[j];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// 2x2 max-pool
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hmaxpool2_fwd_kernel(const _Float16* __restrict__ X, long ldx, int NB, int H, int W, int C,
                                                           _Float16* __restrict__ Y, long ldy) {
  const int q8 = C / 8, Ho = H / 2, Wo = W / 2;
  const long tot = (long)NB * Ho * Wo * q8;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < tot; i += (long)gridDim.x * 256) {
    const int c = (int)(i % q8) * 8; long r = i / q8;
    const int xo = r % Wo; r /= Wo; const int yo = r % Ho; const long n = r / Ho;
    const _Float16* b = X + (((n * H) + 2 * yo) * W + 2 * xo) * ldx + c;
    const f32x8 v00 = ld8h(b), v01 = ld8h(b + ldx), v10 = ld8h(b + (long)W * ldx), v11 = ld8h(b + (long)W * ldx + ldx);
    f32x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = fmaxf(fmaxf(v00[e], v01[e]), fmaxf(v10[e], v11[e]));
    st8h(Y + (((n * Ho) + yo) * Wo + xo) * ldy + c, o);
  }
}
// BatchNorm apply + LeakyReLU of an encoder block's last stage AND the 2x2 max-pool of the result in one pass over the f16
// pre-activation (bn_act_pool_fwd_kernel's form on f16 storage; the f16 inference route, ops.eval_half): a thread owns a 2x2 pixel
// window x V channels (V = 8: 16-byte accesses; V = 4: 8-byte ones, for rows that are not whole 16-byte pieces) - four Z loads,
// four A stores, one pooled store.  Per element the fp32 expression of bn_act_fwd_kernel<_Float16>, rounded once to f16; the
// pooled value is the maximum of the four ROUNDED values in hmaxpool2_fwd_kernel's order - both outputs equal, bit for bit,
// arco_bn_act_fwd_h followed by arco_maxpool2_fwd_h.  A may be the leading channels of a wider buffer (lda > C: concat room).
template <int V>
__global__ __launch_bounds__(256) void hbn_act_pool_fwd_kernel(const _Float16* __restrict__ Z, long ldz, int NB, int H, int W, int C,
                                                              const float* __restrict__ mean, const float* __restrict__ istd,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              float slope, _Float16* __restrict__ Aout, long lda,
                                                              _Float16* __restrict__ Pout, long ldp, int img_per_group) {
  typedef float fv __attribute__((ext_vector_type(V)));
  typedef _Float16 hv __attribute__((ext_vector_type(V)));
  const int qv = C / V, Ho = H / 2, Wo = W / 2;
  const long tot = (long)NB * Ho * Wo * qv;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < tot; i += (long)gridDim.x * 256) {
    const int c = (int)(i % qv) * V; long r = i / qv;
    const int xo = r % Wo; r /= Wo; const int yo = r % Ho; const long n = r / Ho;
    const long g = n / img_per_group;
    fv mu, is, ga, be;
#pragma unroll
    for (int e = 0; e < V; e += 4) {
      const f32x4 m4 = *reinterpret_cast<const f32x4*>(mean + g * C + c + e), i4 = *reinterpret_cast<const f32x4*>(istd + g * C + c + e);
      const f32x4 g4 = *reinterpret_cast<const f32x4*>(gamma + c + e), b4 = *reinterpret_cast<const f32x4*>(beta + c + e);
#pragma unroll
      for (int k = 0; k < 4; ++k) { mu[e + k] = m4[k]; is[e + k] = i4[k]; ga[e + k] = g4[k]; be[e + k] = b4[k]; }
    }
    const long row = ((n * H) + 2 * yo) * W + 2 * xo;
    const long rows[4] = {row, row + 1, row + W, row + W + 1};
    fv z[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) z[u] = __builtin_convertvector(*reinterpret_cast<const hv*>(Z + rows[u] * ldz + c), fv);
    fv o[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      fv a;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        float y = (z[u][e] - mu[e]) * is[e] * ga[e] + be[e];
        y = y >= 0.f ? y : y * slope;
        a[e] = y;
      }
      const hv ah = __builtin_convertvector(a, hv);
      *reinterpret_cast<hv*>(Aout + rows[u] * lda + c) = ah;
      o[u] = __builtin_convertvector(ah, fv);                      // the pooling reads what was stored
    }
    fv m;
#pragma unroll
    for (int e = 0; e < V; ++e) m[e] = fmaxf(fmaxf(o[0][e], o[1][e]), fmaxf(o[2][e], o[3][e]));
    *reinterpret_cast<hv*>(Pout + (((n * Ho) + yo) * Wo + xo) * ldp + c) = __builtin_convertvector(m, hv);
  }
}
// gradient goes to the first maximum in window scan order (as maxpool2_bwd_kernel / torch's saved argmax)
__global__ __launch_bounds__(256) void hmaxpool2_bwd_kernel(const _Float16* __restrict__ X, long ldx, int NB, int H, int W, int C,
                                                           const _Float16* __restrict__ dY, long ldy, _Float16* __restrict__ dX,
                                                           long ldo, const _Float16* __restrict__ add, long lda) {
  const int q8 = C / 8, Ho = H / 2, Wo = W / 2;
  const long tot = (long)NB * Ho * Wo * q8;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < tot; i += (long)gridDim.x * 256) {
    const int c = (int)(i % q8) * 8; long r = i / q8;
    const int xo = r % Wo; r /= Wo; const int yo = r % Ho; const long n = r / Ho;
    const long p00 = ((n * H) + 2 * yo) * W + 2 * xo;
    const long off[4] = {p00, p00 + 1, p00 + W, p00 + W + 1};
    f32x8 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = ld8h(X + off[k] * ldx + c);
    const f32x8 g = ld8h(dY + (((n * Ho) + yo) * Wo + xo) * ldy + c);
    f32x8 o[4];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int best = 0; float bv = v[0][e];
#pragma unroll
      for (int k = 1; k < 4; ++k) if (v[k][e] > bv) { bv = v[k][e]; best = k; }
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k][e] = k == best ? g[e] : 0.f;
    }
    if (add) {           // + the gradient of the other consumer of x (the decoder's skip connection), summed in fp32
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] += ld8h(add + off[k] * lda + c);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) st8h(dX + off[k] * ldo + c, o[k]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// bilinear resize, align_corners = True
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hbilinear_fwd_kernel(const _Float16* __restrict__ X, long ldx, int NB, int Hi, int Wi, int C,
                                                           int Ho, int Wo, _Float16* __restrict__ Y, long ldy) {
  const int q8 = C / 8;
  const float sh = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f, sw = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
  const long tot = (long)NB * Ho * Wo * q8;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < tot; i += (long)gridDim.x * 256) {
    const int c = (int)(i % q8) * 8; long r = i / q8;
    const int xo = r % Wo; r /= Wo; const int yo = r % Ho; const long n = r / Ho;
    int y0, y1, x0, x1; float ly, lx;
    ac_src(yo, sh, Hi, y0, y1, ly); ac_src(xo, sw, Wi, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const _Float16* b = X + (n * Hi) * (long)Wi * ldx + c;
    const f32x8 v00 = ld8h(b + ((long)y0 * Wi + x0) * ldx), v01 = ld8h(b + ((long)y0 * Wi + x1) * ldx);
    const f32x8 v10 = ld8h(b + ((long)y1 * Wi + x0) * ldx), v11 = ld8h(b + ((long)y1 * Wi + x1) * ldx);
    f32x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = hy * (hx * v00[e] + lx * v01[e]) + ly * (hx * v10[e] + lx * v11[e]);
    st8h(Y + (((n * Ho) + yo) * Wo + xo) * ldy + c, o);
  }
}
// adjoint as a gather (no atomics), as bilinear_bwd_kernel: input pixel (yi, xi) collects from the output pixels that reference it
__global__ __launch_bounds__(256) void hbilinear_bwd_kernel(const _Float16* __restrict__ dY, long ldy, int NB, int Hi, int Wi, int C,
                                                           int Ho, int Wo, _Float16* __restrict__ dX, long ldx) {
  const int q8 = C / 8;
  const float sh = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f, sw = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
  const float ish = sh > 0.f ? 1.f / sh : 0.f, isw = sw > 0.f ? 1.f / sw : 0.f;
  const long tot = (long)NB * Hi * Wi * q8;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < tot; i += (long)gridDim.x * 256) {
    const int c = (int)(i % q8) * 8; long r = i / q8;
    const int xi = r % Wi; r /= Wi; const int yi = r % Hi; const long n = r / Hi;
    int ya = sh > 0.f ? (int)floorf((float)(yi - 1) * ish) - 1 : 0, yb = sh > 0.f ? (int)ceilf((float)(yi + 1) * ish) + 1 : Ho - 1;
    int xa = sw > 0.f ? (int)floorf((float)(xi - 1) * isw) - 1 : 0, xb = sw > 0.f ? (int)ceilf((float)(xi + 1) * isw) + 1 : Wo - 1;
    ya = max(ya, 0); yb = min(yb, Ho - 1); xa = max(xa, 0); xb = min(xb, Wo - 1);
    f32x8 acc = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int yo = ya; yo <= yb; ++yo) {
      int y0, y1; float ly; ac_src(yo, sh, Hi, y0, y1, ly);
      float wy = 0.f;
      if (y0 == yi) wy += 1.f - ly;
      if (y1 == yi) wy += ly;
      if (!(y0 == yi || y1 == yi)) continue;
      for (int xo = xa; xo <= xb; ++xo) {
        int x0, x1; float lx; ac_src(xo, sw, Wi, x0, x1, lx);
        float wx = 0.f;
        if (x0 == xi) wx += 1.f - lx;
        if (x1 == xi) wx += lx;
        if (!(x0 == xi || x1 == xi)) continue;
        const f32x8 g = ld8h(dY + (((n * Ho) + yo) * Wo + xo) * ldy + c);
        const float w = wy * wx;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += w * g[e];
      }
    }
    st8h(dX + (((n * Hi) + yi) * Wi + xi) * ldx + c, acc);
  }
}

// 16-byte lanes: every pointer 16-byte aligned, every row stride a multiple of 8 elements
static bool arco_h8_ok(std::initializer_list<const void*> ptrs, std::initializer_list<long> lds) {
  for (const void* p : ptrs) if (!p || (reinterpret_cast<uintptr_t>(p) & 15) != 0) return false;
  for (long l : lds) if ((l & 7) != 0) return false;
  return true;
}

extern "C" {

// number of BatchNorm partial slabs per channel that arco_conv3x3_image_fwd_h writes (= its workgroups)
int arco_conv3x3_image_mblocks_h(int NB, int H, int W, int stat_groups) {
  const int n_grp = stat_groups > 1 ? stat_groups : 1;
  if (NB <= 0 || H <= 0 || W <= 0 || NB % n_grp != 0) return ARCO_ERR_ARG;
  return (int)himage_blocks(NB, H, W, n_grp);
}
// out (f16) [pix][0..N) = conv3x3(in (fp32 image, K <= 4 channels); Wp: the fp32 forward pack [9][16][16]) + bias; N <= 16
int arco_conv3x3_image_fwd_h(const float* in, long ld_in, int K, const float* Wp, int N, void* out, long ld_out, const float* bias,
                             float* stat_sum, float* stat_sq, int NB, int H, int W, int stat_groups, void* stream) {
  const int n_grp = stat_groups > 1 ? stat_groups : 1;
  ARCO_CHECK_ARG(in && Wp && out && K >= 1 && K <= 4 && N >= 4 && N <= 16 && (N & 3) == 0 && (ld_out & 3) == 0 && ld_in >= K &&
                 NB > 0 && H > 0 && W > 0 && NB % n_grp == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0 &&
                 (stat_sum == nullptr) == (stat_sq == nullptr));
  const long blocks = himage_blocks(NB, H, W, n_grp);
  hipLaunchKernelGGL(himage_conv_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), in, ld_in, K, Wp, N, 16, 16, bias,
                     reinterpret_cast<_Float16*>(out), ld_out, NB, H, W, stat_sum, stat_sq, n_grp);
  return arco_launch_status();
}
// dW [16][K][3][3] (+)= sum_pix dZ (f16, 16 channels) x in (fp32 image); ws sized by arco_wgrad_ws_floats(16, K, 9, NB * H * W)
int arco_conv3x3_image_wgrad_h(const void* dZ, long ld_dz, int Cout, const float* in, long ld_in, int K, int NB, int H, int W,
                               float* ws, float* dW, int accumulate, void* stream) {
  ARCO_CHECK_ARG(dZ && in && ws && dW && K >= 1 && K <= 4 && ld_in >= K && NB > 0 && H > 0 && W > 0 && Cout > 0 && ld_dz >= Cout &&
                 (accumulate == 0 || accumulate == 1));
  arco_note_wgrad_route(0);
  WgradPlan p;       // (the slab count never exceeds what arco_wgrad_ws_floats reserves: wgrad_plan clamps it)
  const int rc = wgrad_plan(1, 9, NB, 1, H, W, K, Cout, ld_dz, ld_in, 4, false, 0, (reinterpret_cast<uintptr_t>(dZ) & 15) == 0, p);
  if (rc != ARCO_OK) return rc;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(himage_wgrad_kernel, dim3((unsigned)p.slabs), dim3(256), 0, st, reinterpret_cast<const _Float16*>(dZ), ld_dz, in,
                     ld_in, K, NB, H, W, ws);
  arco_note_wgrad_route(p.route);
  launch_wgrad_reduce(st, ws, (int)p.slabs, 9, p.CoutPad, p.CinPad, Cout, K, dW, accumulate);
  return arco_launch_status();
}

int arco_maxpool2_fwd_h(const void* X, long ldx, int NB, int H, int W, int C, void* Y, long ldy, void* stream) {
  ARCO_CHECK_ARG(C > 0 && (C & 7) == 0 && (H & 1) == 0 && (W & 1) == 0 && NB > 0 && arco_h8_ok({X, Y}, {ldx, ldy}));
  hipLaunchKernelGGL(hmaxpool2_fwd_kernel, dim3(uh_grid((long)NB * (H / 2) * (W / 2) * (C / 8))), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const _Float16*>(X), ldx, NB, H, W, C, reinterpret_cast<_Float16*>(Y), ldy);
  return arco_launch_status();
}
// A (f16) [pix][0..C) = lrelu(BN(Z (f16))) and P (f16) = maxpool2(A) in one pass; mean / istd [groups][C], gamma / beta [C], fp32.
// 16-byte lanes where every pointer and row stride allows them, else 8-byte lanes (C and the strides multiples of 4).
int arco_bn_act_pool_fwd_h(const void* Z, long ldz, int NB, int H, int W, int C, const float* mean, const float* istd,
                           const float* gamma, const float* beta, float slope, void* A, long lda, void* P, long ldp, int groups,
                           void* stream) {
  if (groups < 1) groups = 1;
  ARCO_CHECK_ARG(Z && mean && istd && gamma && beta && A && P && NB > 0 && H > 0 && W > 0 && C > 0 && (C & 3) == 0 && (H & 1) == 0 &&
                 (W & 1) == 0 && NB % groups == 0 && ldz >= C && lda >= C && ldp >= C && ((ldz | lda | ldp) & 3) == 0);
  for (const void* p : {Z, (const void*)A, (const void*)P}) ARCO_CHECK_ARG((reinterpret_cast<uintptr_t>(p) & 7) == 0);
  for (const void* p : {(const void*)mean, (const void*)istd, (const void*)gamma, (const void*)beta})
    ARCO_CHECK_ARG((reinterpret_cast<uintptr_t>(p) & 15) == 0);
  const _Float16* z = reinterpret_cast<const _Float16*>(Z);
  _Float16* a = reinterpret_cast<_Float16*>(A); _Float16* p = reinterpret_cast<_Float16*>(P);
  if ((C & 7) == 0 && arco_h8_ok({Z, A, P}, {ldz, lda, ldp}))
    hipLaunchKernelGGL(hbn_act_pool_fwd_kernel<8>, dim3(uh_grid((long)NB * (H / 2) * (W / 2) * (C / 8))), dim3(256), 0, as_stream(stream),
                       z, ldz, NB, H, W, C, mean, istd, gamma, beta, slope, a, lda, p, ldp, NB / groups);
  else
    hipLaunchKernelGGL(hbn_act_pool_fwd_kernel<4>, dim3(uh_grid((long)NB * (H / 2) * (W / 2) * (C / 4))), dim3(256), 0, as_stream(stream),
                       z, ldz, NB, H, W, C, mean, istd, gamma, beta, slope, a, lda, p, ldp, NB / groups);
  return arco_launch_status();
}
int arco_maxpool2_bwd_h(const void* X, long ldx, int NB, int H, int W, int C, const void* dY, long ldy, void* dX, long ldo,
                        void* stream) {
  ARCO_CHECK_ARG(C > 0 && (C & 7) == 0 && (H & 1) == 0 && (W & 1) == 0 && NB > 0 && arco_h8_ok({X, dY, dX}, {ldx, ldy, ldo}));
  hipLaunchKernelGGL(hmaxpool2_bwd_kernel, dim3(uh_grid((long)NB * (H / 2) * (W / 2) * (C / 8))), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const _Float16*>(X), ldx, NB, H, W, C, reinterpret_cast<const _Float16*>(dY), ldy,
                     reinterpret_cast<_Float16*>(dX), ldo, (const _Float16*)nullptr, 0l);
  return arco_launch_status();
}
// dX = maxpool2_bwd(dY) + add  (add: the gradient x receives from its other consumer, the U-Net skip connection)
int arco_maxpool2_bwd_add_h(const void* X, long ldx, int NB, int H, int W, int C, const void* dY, long ldy, const void* add,
                            long ld_add, void* dX, long ldo, void* stream) {
  ARCO_CHECK_ARG(C > 0 && (C & 7) == 0 && (H & 1) == 0 && (W & 1) == 0 && NB > 0 &&
                 arco_h8_ok({X, dY, add, dX}, {ldx, ldy, ld_add, ldo}));
  hipLaunchKernelGGL(hmaxpool2_bwd_kernel, dim3(uh_grid((long)NB * (H / 2) * (W / 2) * (C / 8))), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const _Float16*>(X), ldx, NB, H, W, C, reinterpret_cast<const _Float16*>(dY), ldy,
                     reinterpret_cast<_Float16*>(dX), ldo, reinterpret_cast<const _Float16*>(add), ld_add);
  return arco_launch_status();
}
int arco_bilinear_fwd_h(const void* X, long ldx, int NB, int Hi, int Wi, int C, int Ho, int Wo, void* Y, long ldy, void* stream) {
  ARCO_CHECK_ARG(C > 0 && (C & 7) == 0 && NB > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && arco_h8_ok({X, Y}, {ldx, ldy}));
  hipLaunchKernelGGL(hbilinear_fwd_kernel, dim3(uh_grid((long)NB * Ho * Wo * (C / 8))), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const _Float16*>(X), ldx, NB, Hi, Wi, C, Ho, Wo, reinterpret_cast<_Float16*>(Y), ldy);
  return arco_launch_status();
}
int arco_bilinear_bwd_h(const void* dY, long ldy, int NB, int Hi, int Wi, int C, int Ho, int Wo, void* dX, long ldx, void* stream) {
  ARCO_CHECK_ARG(C > 0 && (C & 7) == 0 && NB > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && arco_h8_ok({dY, dX}, {ldy, ldx}));
  hipLaunchKernelGGL(hbilinear_bwd_kernel, dim3(uh_grid((long)NB * Hi * Wi * (C / 8))), dim3(256), 0, as_stream(stream),
                     reinterpret_cast<const _Float16*>(dY), ldy, NB, Hi, Wi, C, Ho, Wo, reinterpret_cast<_Float16*>(dX), ldx);
  return arco_launch_status();
}

}  // extern "C"
