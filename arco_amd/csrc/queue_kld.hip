// The KL-divergence-to-queue loss of stage 1 (arco_amd/stage1.py queue_kld(route="fused"), pretrain_2D / pretrain_3D --kld fused):
//   loss = F.kl_div(F.log_softmax(cs / Ts, 1), F.softmax(ct / Tt, 1), 'batchmean') over two [N, L] matrices of raw cosines,
//   arco_queue_kld_fwd   one pass over each matrix: per row lse_s, lse_t, KL -> stats [N, 3] float64; then the loss in a small second launch
//   arco_queue_kld_bwd   elementwise from the statistics: d loss / d cs, d loss / d ct (either may be written over its own matrix)
//
// Forward, per row, with s = cs / Ts, t = ct / Tt: every thread keeps the largest cosines of ITS elements and, relative to ms = max s, mt = max t,
//   zs = sum e^(s - ms),  zt = sum e^(t - mt),  w = sum e^(t - mt) ((t - mt) - (s - ms))
// (an online softmax: when a maximum moves the sums are rescaled, `rebase`).  The thread states are merged across the wave by a butterfly
// and across the workgroup through 5 doubles of LDS per wave, thread 0 adding the waves in ascending order: the order is a function of L
// and the launch geometry alone, there is no atomic, two runs give the same bits.  Then
//   lse_s = ms + log zs,  lse_t = mt + log zt,  KL = w / zt - log zt + log zs          (sum_j p_ij = 1)
// The exponentials are fp32; the differences s - ms = (cosine - largest cosine) / T and the three sums are float64: nothing of the size of
// 1 / T is rounded to fp32, the row maximum's term is exactly 1 as in a two-pass softmax, and KL_i is a weighted mean of exactly the
// differences the backward kernel subtracts it from (a one-spike teacher's gradient is 0, not the rounding of a logit of 100).  A term
// whose e^(t - mt) underflows contributes exactly 0 (F.kl_div's xlogy convention); a non-finite cosine makes its row's statistics and the
// loss non-finite (fmaxf skips a NaN, the exponential of the difference does not).  cs == ct with equal temperatures gives w == 0 and
// lse_s == lse_t bit for bit: KL == 0.
//
// Geometry: rows longer than QK_SHORT_L take one workgroup of 256 threads each; shorter ones (the latent term: L = K = 36) one wave each,
// four rows per workgroup.  16-byte loads where L, both row strides and both pointers are multiples of 4 floats / 16 bytes, a scalar path
// otherwise.
#pragma clang fp contract(off)
#include "common.h"
#include <math.h>

namespace {

constexpr int QK_THREADS = 256;
constexpr int QK_WAVES = QK_THREADS / 64;
constexpr long QK_SHORT_L = 512;          // rows up to this length: one wave per row (8 elements or 2 vector loads per lane at the switch)
constexpr int QK_SUM_THREADS = 256;

struct RowState {
  float ms, mt;          // the largest raw cosines so far; the sums are relative to ms / Ts and mt / Tt
  double zs, zt, w;      // float64 sums of fp32 exponentials (and of their products with the float64 differences)
};

__device__ __forceinline__ RowState empty_state() { return RowState{-INFINITY, -INFINITY, 0.0, 0.0, 0.0}; }

// the same sums relative to the maxima Ms >= st.ms, Mt >= st.mt.  A state without elements (m = -inf, z = 0) only takes the maxima: its
// shifts are infinite.  Every other state holds the term of its own maximum, e^0 = 1, or a NaN, so that neither z is 0.  w and zt take
// the SAME factor: their quotient, the weighted mean that KL_i is made of, does not see its rounding.
__device__ __forceinline__ void rebase(RowState& st, float Ms, float Mt, float inv_ts, float inv_tt) {
  if (st.zs != 0.0 || st.zt != 0.0) {
    const double ds = ((double)Ms - (double)st.ms) * (double)inv_ts, dt = ((double)Mt - (double)st.mt) * (double)inv_tt;
    const double ft = (double)expf((float)-dt);
    st.w = ft * (st.w + (ds - dt) * st.zt);
    st.zt = ft * st.zt;
    st.zs = (double)expf((float)-ds) * st.zs;
  }
  st.ms = Ms;
  st.mt = Mt;
}

// b = s - max s and a = t - max t as (cosine - largest cosine) / T in float64: the difference of two floats is exact there, so the
// maximum's own term is e^0 = 1 exactly and a - b is the float64 value the backward kernel computes again from the lse's.  Only the
// exponentials are fp32; their rounding reaches KL_i through the spread of a - b about its weighted mean alone, not through its size.
__device__ __forceinline__ void add_element(RowState& st, float cs, float ct, float inv_ts, float inv_tt) {
  const double b = ((double)cs - (double)st.ms) * (double)inv_ts, a = ((double)ct - (double)st.mt) * (double)inv_tt;
  const double e = (double)expf((float)a);
  st.zs += (double)expf((float)b);
  st.zt += e;
  st.w += e * (a - b);
}

__device__ __forceinline__ RowState merge(RowState x, RowState y, float inv_ts, float inv_tt) {
  const float Ms = fmaxf(x.ms, y.ms), Mt = fmaxf(x.mt, y.mt);
  rebase(x, Ms, Mt, inv_ts, inv_tt);
  rebase(y, Ms, Mt, inv_ts, inv_tt);
  return RowState{Ms, Mt, x.zs + y.zs, x.zt + y.zt, x.w + y.w};
}

__device__ __forceinline__ RowState wave_merge(RowState st, float inv_ts, float inv_tt) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    RowState other{__shfl_xor(st.ms, o, 64), __shfl_xor(st.mt, o, 64), __shfl_xor(st.zs, o, 64), __shfl_xor(st.zt, o, 64), __shfl_xor(st.w, o, 64)};
    st = merge(st, other, inv_ts, inv_tt);          // both partners add the same two operands: every lane ends with the same bits
  }
  return st;
}

// the elements j = first, first + stride, ... of one row (VEC: groups of four, j counts floats)
template <bool VEC>
__device__ __forceinline__ RowState scan_row(const float* __restrict__ cs, const float* __restrict__ ct, long L, int first, int stride,
                                             float inv_ts, float inv_tt) {
  RowState st = empty_state();
  if (VEC) {
    for (long j = 4L * first; j < L; j += 4L * stride) {
      const f32x4 vs = *reinterpret_cast<const f32x4*>(cs + j), vt = *reinterpret_cast<const f32x4*>(ct + j);
      const float cms = fmaxf(fmaxf(vs[0], vs[1]), fmaxf(vs[2], vs[3])), cmt = fmaxf(fmaxf(vt[0], vt[1]), fmaxf(vt[2], vt[3]));
      if (cms > st.ms || cmt > st.mt) rebase(st, fmaxf(st.ms, cms), fmaxf(st.mt, cmt), inv_ts, inv_tt);
#pragma unroll
      for (int e = 0; e < 4; ++e) add_element(st, vs[e], vt[e], inv_ts, inv_tt);
    }
  } else {
    for (long j = first; j < L; j += stride) {
      const float xs = cs[j], xt = ct[j];
      if (xs > st.ms || xt > st.mt) rebase(st, fmaxf(st.ms, xs), fmaxf(st.mt, xt), inv_ts, inv_tt);
      add_element(st, xs, xt, inv_ts, inv_tt);
    }
  }
  return st;
}

// lse = (largest cosine) / T, an exact product in float64, + log z
__device__ __forceinline__ void write_stats(const RowState& st, float inv_ts, float inv_tt, double* __restrict__ out) {
  const double lzs = log(st.zs), lzt = log(st.zt);
  out[0] = (double)st.ms * (double)inv_ts + lzs;
  out[1] = (double)st.mt * (double)inv_tt + lzt;
  out[2] = st.w / st.zt - lzt + lzs;
}

// one workgroup per row
template <bool VEC>
__global__ __launch_bounds__(QK_THREADS) void queue_kld_fwd_long_kernel(const float* __restrict__ cs, const float* __restrict__ ct, long L,
                                                                        long ld_s, long ld_t, float inv_ts, float inv_tt,
                                                                        double* __restrict__ stats) {
  __shared__ double part[QK_WAVES][5];
  const long row = blockIdx.x;
  RowState st = scan_row<VEC>(cs + row * ld_s, ct + row * ld_t, L, threadIdx.x, QK_THREADS, inv_ts, inv_tt);
  st = wave_merge(st, inv_ts, inv_tt);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[wave][0] = (double)st.ms; part[wave][1] = (double)st.mt; part[wave][2] = st.zs; part[wave][3] = st.zt; part[wave][4] = st.w;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int v = 1; v < QK_WAVES; ++v) st = merge(st, RowState{(float)part[v][0], (float)part[v][1], part[v][2], part[v][3], part[v][4]}, inv_ts, inv_tt);
    write_stats(st, inv_ts, inv_tt, stats + 3 * row);
  }
}

// one wave per row, QK_WAVES rows per workgroup
template <bool VEC>
__global__ __launch_bounds__(QK_THREADS) void queue_kld_fwd_short_kernel(const float* __restrict__ cs, const float* __restrict__ ct, long N,
                                                                         long L, long ld_s, long ld_t, float inv_ts, float inv_tt,
                                                                         double* __restrict__ stats) {
  const long row = (long)blockIdx.x * QK_WAVES + (threadIdx.x >> 6);
  if (row >= N) return;          // the whole wave leaves: the butterfly below never waits for it
  const int lane = threadIdx.x & 63;
  RowState st = wave_merge(scan_row<VEC>(cs + row * ld_s, ct + row * ld_t, L, lane, 64, inv_ts, inv_tt), inv_ts, inv_tt);
  if (lane == 0) write_stats(st, inv_ts, inv_tt, stats + 3 * row);
}

// loss = (sum of KL_i in float64: thread u adds the rows u, u + 256, ... ascending, then a tree over the 256 partial sums) / N, rounded once
__global__ __launch_bounds__(QK_SUM_THREADS) void queue_kld_loss_kernel(const double* __restrict__ stats, long N, float* __restrict__ loss) {
  __shared__ double part[QK_SUM_THREADS];
  double acc = 0.0;
  for (long i = threadIdx.x; i < N; i += QK_SUM_THREADS) acc += stats[3 * i + 2];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int o = QK_SUM_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(part[0] / (double)N);
}

struct RowGrad {
  double lse_s, lse_t, kl;
  float gs, gt;
};

__device__ __forceinline__ RowGrad row_grad(const double* __restrict__ stats, long row, const float* __restrict__ g, long N, float inv_ts,
                                            float inv_tt) {
  RowGrad r;
  r.lse_s = stats[3 * row]; r.lse_t = stats[3 * row + 1]; r.kl = stats[3 * row + 2];
  const double gn = (double)g[0] / (double)N;
  r.gs = (float)(gn * (double)inv_ts);
  r.gt = (float)(gn * (double)inv_tt);
  return r;
}

// log softmax(s)_ij, log p_ij and (log p - log q) - KL_i in float64 - the forward's a - b minus its weighted mean, to 1e-13, however large
// the logits are; the exponentials and the products in fp32
template <bool WANT_S, bool WANT_T>
__device__ __forceinline__ void grad_element(const RowGrad& r, float cs, float ct, float inv_ts, float inv_tt, float& ds, float& dt) {
  const double ls = (double)cs * (double)inv_ts - r.lse_s, lt = (double)ct * (double)inv_tt - r.lse_t;
  const float p = expf((float)lt);
  if (WANT_S) ds = r.gs * (expf((float)ls) - p);
  if (WANT_T) dt = r.gt * (p * (float)((lt - ls) - r.kl));
}

// Row `row`, elements first, first + stride, ...  dcs / dct may be cs / ct themselves: a thread reads its elements of both matrices before
// it writes either, and no other thread touches them - hence no __restrict__ on the four.
template <bool VEC, bool WANT_S, bool WANT_T>
__device__ __forceinline__ void grad_row(const float* cs, const float* ct, long L, int first, int stride, float inv_ts, float inv_tt,
                                         const RowGrad& r, float* dcs, float* dct) {
  if (VEC) {
    for (long j = 4L * first; j < L; j += 4L * stride) {
      const f32x4 vs = *reinterpret_cast<const f32x4*>(cs + j), vt = *reinterpret_cast<const f32x4*>(ct + j);
      f32x4 os, ot;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float a = 0.f, b = 0.f;
        grad_element<WANT_S, WANT_T>(r, vs[e], vt[e], inv_ts, inv_tt, a, b);
        os[e] = a; ot[e] = b;
      }
      if (WANT_S) *reinterpret_cast<f32x4*>(dcs + j) = os;
      if (WANT_T) *reinterpret_cast<f32x4*>(dct + j) = ot;
    }
  } else {
    for (long j = first; j < L; j += stride) {
      float a = 0.f, b = 0.f;
      grad_element<WANT_S, WANT_T>(r, cs[j], ct[j], inv_ts, inv_tt, a, b);
      if (WANT_S) dcs[j] = a;
      if (WANT_T) dct[j] = b;
    }
  }
}

// SHORT: one wave per row, QK_WAVES rows per workgroup; else one workgroup per row
template <bool VEC, bool WANT_S, bool WANT_T, bool SHORT>
__global__ __launch_bounds__(QK_THREADS) void queue_kld_bwd_kernel(const float* cs, const float* ct, long N, long L, long ld_s, long ld_t,
                                                                   float inv_ts, float inv_tt, const double* __restrict__ stats,
                                                                   const float* __restrict__ g, float* dcs, long ld_ds, float* dct, long ld_dt) {
  const long row = SHORT ? (long)blockIdx.x * QK_WAVES + (threadIdx.x >> 6) : (long)blockIdx.x;
  if (row >= N) return;
  const RowGrad r = row_grad(stats, row, g, N, inv_ts, inv_tt);
  grad_row<VEC, WANT_S, WANT_T>(cs + row * ld_s, ct + row * ld_t, L, SHORT ? (int)(threadIdx.x & 63) : (int)threadIdx.x, SHORT ? 64 : QK_THREADS,
                                inv_ts, inv_tt, r, WANT_S ? dcs + row * ld_ds : nullptr, WANT_T ? dct + row * ld_dt : nullptr);
}

inline bool vec_ok(const void* p, long ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0; }

inline bool shape_ok(long N, long L, long ld_s, long ld_t, float inv_ts, float inv_tt) {
  // grid.x holds the row count; a row stride times a row number stays inside a long by a wide margin
  return N >= 1 && N <= 0x7fffffffL && L >= 1 && L <= 0x7fffffffL && ld_s >= L && ld_t >= L && ld_s <= 0x7fffffffL && ld_t <= 0x7fffffffL &&
         inv_ts > 0.f && inv_tt > 0.f && inv_ts < INFINITY && inv_tt < INFINITY;
}

template <bool VEC, bool WANT_S, bool WANT_T>
void launch_bwd(bool is_short, hipStream_t st, const float* cs, const float* ct, long N, long L, long ld_s, long ld_t, float inv_ts, float inv_tt,
                const double* stats, const float* g, float* dcs, long ld_ds, float* dct, long ld_dt) {
  if (is_short)
    hipLaunchKernelGGL((queue_kld_bwd_kernel<VEC, WANT_S, WANT_T, true>), dim3((unsigned)((N + QK_WAVES - 1) / QK_WAVES)), dim3(QK_THREADS), 0, st,
                       cs, ct, N, L, ld_s, ld_t, inv_ts, inv_tt, stats, g, dcs, ld_ds, dct, ld_dt);
  else
    hipLaunchKernelGGL((queue_kld_bwd_kernel<VEC, WANT_S, WANT_T, false>), dim3((unsigned)N), dim3(QK_THREADS), 0, st,
                       cs, ct, N, L, ld_s, ld_t, inv_ts, inv_tt, stats, g, dcs, ld_ds, dct, ld_dt);
}

template <bool VEC>
void launch_bwd_want(bool is_short, hipStream_t st, const float* cs, const float* ct, long N, long L, long ld_s, long ld_t, float inv_ts,
                     float inv_tt, const double* stats, const float* g, float* dcs, long ld_ds, float* dct, long ld_dt) {
  if (dcs && dct) launch_bwd<VEC, true, true>(is_short, st, cs, ct, N, L, ld_s, ld_t, inv_ts, inv_tt, stats, g, dcs, ld_ds, dct, ld_dt);
  else if (dcs) launch_bwd<VEC, true, false>(is_short, st, cs, ct, N, L, ld_s, ld_t, inv_ts, inv_tt, stats, g, dcs, ld_ds, dct, ld_dt);
  else launch_bwd<VEC, false, true>(is_short, st, cs, ct, N, L, ld_s, ld_t, inv_ts, inv_tt, stats, g, dcs, ld_ds, dct, ld_dt);
}

}  // namespace

extern "C" {

long arco_queue_kld_short_max(void) { return QK_SHORT_L; }

int arco_queue_kld_fwd(const float* cs, const float* ct, long N, long L, long ld_s, long ld_t, float inv_ts, float inv_tt, double* stats,
                       float* loss, void* stream) {
  ARCO_CHECK_ARG(cs && ct && stats && loss);
  ARCO_CHECK_ARG(shape_ok(N, L, ld_s, ld_t, inv_ts, inv_tt));
  const bool vec = L % 4 == 0 && vec_ok(cs, ld_s) && vec_ok(ct, ld_t);
  hipStream_t st = as_stream(stream);
  if (L <= QK_SHORT_L) {
    const dim3 grid((unsigned)((N + QK_WAVES - 1) / QK_WAVES));
    if (vec) hipLaunchKernelGGL(queue_kld_fwd_short_kernel<true>, grid, dim3(QK_THREADS), 0, st, cs, ct, N, L, ld_s, ld_t, inv_ts, inv_tt, stats);
    else hipLaunchKernelGGL(queue_kld_fwd_short_kernel<false>, grid, dim3(QK_THREADS), 0, st, cs, ct, N, L, ld_s, ld_t, inv_ts, inv_tt, stats);
  } else {
    if (vec) hipLaunchKernelGGL(queue_kld_fwd_long_kernel<true>, dim3((unsigned)N), dim3(QK_THREADS), 0, st, cs, ct, L, ld_s, ld_t, inv_ts, inv_tt, stats);
    else hipLaunchKernelGGL(queue_kld_fwd_long_kernel<false>, dim3((unsigned)N), dim3(QK_THREADS), 0, st, cs, ct, L, ld_s, ld_t, inv_ts, inv_tt, stats);
  }
  hipLaunchKernelGGL(queue_kld_loss_kernel, dim3(1), dim3(QK_SUM_THREADS), 0, st, stats, N, loss);
  return arco_launch_status();
}

int arco_queue_kld_bwd(const float* cs, const float* ct, long N, long L, long ld_s, long ld_t, float inv_ts, float inv_tt, const double* stats,
                       const float* g, float* dcs, long ld_ds, float* dct, long ld_dt, void* stream) {
  ARCO_CHECK_ARG(cs && ct && stats && g && (dcs || dct));
  ARCO_CHECK_ARG(shape_ok(N, L, ld_s, ld_t, inv_ts, inv_tt));
  ARCO_CHECK_ARG((!dcs || (ld_ds >= L && ld_ds <= 0x7fffffffL)) && (!dct || (ld_dt >= L && ld_dt <= 0x7fffffffL)));
  // the one aliasing taken: a gradient written over its own matrix, with that matrix's row stride
  ARCO_CHECK_ARG(dcs != ct && dct != cs && (dcs != dct || !dcs));
  ARCO_CHECK_ARG((dcs != cs || ld_ds == ld_s) && (dct != ct || ld_dt == ld_t));
  const bool vec = L % 4 == 0 && vec_ok(cs, ld_s) && vec_ok(ct, ld_t) && (!dcs || vec_ok(dcs, ld_ds)) && (!dct || vec_ok(dct, ld_dt));
  const bool is_short = L <= QK_SHORT_L;
  hipStream_t st = as_stream(stream);
  if (vec) launch_bwd_want<true>(is_short, st, cs, ct, N, L, ld_s, ld_t, inv_ts, inv_tt, stats, g, dcs, ld_ds, dct, ld_dt);
  else launch_bwd_want<false>(is_short, st, cs, ct, N, L, ld_s, ld_t, inv_ts, inv_tt, stats, g, dcs, ld_ds, dct, ld_dt);
  return arco_launch_status();
}

}  // extern "C"
