// The patch-wise output heads of stage 1 as one kernel each way (arco_amd/stage1.py patch_heads(route="fused"), pretrain_2D / pretrain_3D
// --patch_heads fused): the adaptive average pooling of patch_pool.hip followed by the heads' 1 to 4 pointwise (1x1) layers, which have no
// non-linearity between them.
//   arco_patch_head_fwd            x [B, C, n...] -> pooled [P, B, C, pool...] (saved for the backward) and y [P * B, C_L, pool...]
//   arco_patch_head_bwd            pooled, gy [P * B, C_L, pool...] -> d0 [P, B, C, pool...] (optional) and one slab of float64 parameter-
//                                  gradient partials per workgroup
//   arco_patch_head_wgrad_finish   the slabs summed in ascending order in float64, rounded once to fp32
// The geometry is patch_geom.h's.  A POSITION is one (patch p, batch b, cell) triple, q = (p * B + b) * cells + cell, cells = pool^nd;
// one thread per position.  With the widths C = c_0, c_1 .. c_L and a_0 = the pooled values of the position (patch_pool_fwd_kernel's
// window sum and divide, the same bits), layer k = 1 .. L computes in fp32, every operation rounded on its own (no fused multiply-add),
//   a_k[j] = b_k[j] (0.f without a bias); then for i ascending: a_k[j] = a_k[j] + W_k[j, i] * a_{k-1}[i]
// and y = a_L.  The weight matrices are never multiplied together: every layer has a gradient of its own.  Backward, per position:
// a_0 .. a_{L-1} are computed again from pooled with the same operations, d_L = gy, and for k = L .. 1
//   d_{k-1}[i] = 0.f; then for j ascending: d_{k-1}[i] = d_{k-1}[i] + W_k[j, i] * d_k[j]
//   dW_k[j, i] += (double)d_k[j] * (double)a_{k-1}[i] (exact in float64), db_k[j] += (double)d_k[j].
// ORDER of the parameter sums (no atomics; the grid depends on the position count and the width tier alone, so two runs give the same
// bits): the block stages d_k and a_{k-1} of its T positions in LDS; lane l of a wave owns the parameters l, l + 64, ... of the layer
// and adds its wave's 64 positions in ascending lane order to a float64 accumulator that it keeps over all of the block's passes; at the
// end every wave puts its accumulators into an LDS slot of its own, the slots are added in ascending wave order into the block's slab,
// and arco_patch_head_wgrad_finish adds the slabs in ascending block order.
// The kernels are instantiated for the width tiers 8 / 16 / 32 (the largest of the widths rounded up).  The forward's activation vectors
// are register arrays, its loops fully unrolled with bodies predicated on the runtime widths, so no index is a runtime value; the
// backward's are LDS images (see patch_head_bwd_kernel).  No instantiation uses scratch memory (hipcc -Rpass-analysis=kernel-resource-usage).
#pragma clang fp contract(off)
#include "patch_geom.h"

namespace {

#define PH_MAX_LAYERS 4
#define PH_MAX_WIDTH 32
#define PH_BWD_MAX_BLOCKS 512        // slabs at most: the finish kernel adds them one after the other

struct Chain {
  const float* w[PH_MAX_LAYERS];     // W_k [c_k, c_{k-1}] row-major (a Conv weight [out, in, 1, 1(, 1)])
  const float* b[PH_MAX_LAYERS];     // null: no bias
  int width[PH_MAX_LAYERS + 1];      // c_0 .. c_L
  int layers;
};
// the layer number as a type: a generic lambda called once per layer has the number as a compile-time value (a loop over the layers
// is too large for the unroller at the top tier, and a runtime layer number would put the activation arrays into scratch memory)
template <int K> struct LayerNo { static constexpr int value = K; };
using K0 = LayerNo<0>; using K1 = LayerNo<1>; using K2 = LayerNo<2>; using K3 = LayerNo<3>;
struct ChainGrads { float* w[PH_MAX_LAYERS]; float* b[PH_MAX_LAYERS]; };      // null: not wanted

// LDS image of the chain for the tier W: layer k (from 0) at k * (W * W + W): its weights [c_{k+1}][c_k] packed, its bias at W * W
// (zeros without one).  Every k is a compile-time value: the by-value Chain is never indexed by a runtime one.
template <int W, int T>
__device__ __forceinline__ void load_chain(const Chain& ch, float* sw) {
  constexpr int NPL = W * W + W;
#pragma unroll
  for (int k = 0; k < PH_MAX_LAYERS; ++k) {
    if (k < ch.layers) {
      const int win = ch.width[k], wout = ch.width[k + 1];
      for (int e = threadIdx.x; e < wout * win; e += T) sw[k * NPL + e] = ch.w[k][e];
      for (int e = threadIdx.x; e < wout; e += T) sw[k * NPL + W * W + e] = ch.b[k] ? ch.b[k][e] : 0.f;
    }
  }
  __syncthreads();
}

// out[j] = bias[j]; out[j] = out[j] + W[j, i] * in[i] for i ascending (j < wout, i < win); out[j] = 0.f for j >= wout
template <int W>
__device__ __forceinline__ void layer_fwd(const float* sw, int win, int wout, const float (&in)[W], float (&out)[W]) {
#pragma unroll
  for (int j = 0; j < W; ++j) {
    float acc = 0.f;
    if (j < wout) {
      acc = sw[W * W + j];
#pragma unroll
      for (int i = 0; i < W; ++i)
        if (i < win) acc = acc + sw[j * win + i] * in[i];
    }
    out[j] = acc;
  }
}

template <int W>
__global__ __launch_bounds__(PP_THREADS) void patch_head_fwd_kernel(const float* __restrict__ x, Geom g, Chain ch, long total,
                                                                    float* __restrict__ pooled, float* __restrict__ y) {
  constexpr int NPL = W * W + W;
  __shared__ float sw[PH_MAX_LAYERS * NPL];
  load_chain<W, PP_THREADS>(ch, sw);
  const Axis a0 = g.a[0], a1 = g.a[1], a2 = g.a[2];
  const long cells = (long)a0.pool * a1.pool * a2.pool, vol = (long)a0.n * a1.n * a2.n;
  const int C = ch.width[0];
  for (long q = (long)blockIdx.x * PP_THREADS + threadIdx.x; q < total; q += (long)gridDim.x * PP_THREADS) {
    const long cell = q % cells, pb = q / cells;
    long r = cell;
    const int i2 = (int)(r % a2.pool); r /= a2.pool;
    const int i1 = (int)(r % a1.pool); r /= a1.pool;
    const int i0 = (int)r;
    r = pb;
    const int b = (int)(r % g.B); r /= g.B;
    const int p2 = (int)(r % a2.np); r /= a2.np;
    const int p1 = (int)(r % a1.np); r /= a1.np;
    const int p0 = (int)r;
    const Win w = cell_window(g, p0, p1, p2, i0, i1, i2);
    float a[W], t[W];
#pragma unroll
    for (int c = 0; c < W; ++c) {
      a[c] = 0.f;
      if (c < C) {
        a[c] = window_mean(x + ((long)b * C + c) * vol, g, w);
        pooled[(pb * C + c) * cells + cell] = a[c];
      }
    }
    auto layer = [&](auto kc) {
      constexpr int k = decltype(kc)::value;
      if (k < ch.layers) {
        layer_fwd<W>(sw + k * NPL, ch.width[k], ch.width[k + 1], a, t);
#pragma unroll
        for (int j = 0; j < W; ++j) a[j] = t[j];
      }
    };
    layer(K0{}); layer(K1{}); layer(K2{}); layer(K3{});
    int cl = C;
#pragma unroll
    for (int k = 0; k < PH_MAX_LAYERS; ++k)
      if (k < ch.layers) cl = ch.width[k + 1];
#pragma unroll
    for (int j = 0; j < W; ++j)
      if (j < cl) y[(pb * cl + j) * cells + cell] = a[j];
  }
}

// The backward keeps the activation vectors in LDS, not in registers: a_0 .. a_3 and d of a position are 5 * W floats (160 at the top
// tier) beside up to 68 float64 accumulators a lane, which is more than the register file holds, and the parameter sums read the vectors
// of OTHER positions anyway.  Five [W][T + 1] images (row r of thread t at r * (T + 1) + t: a thread's own column is free of bank
// conflicts, and so are the parameter sums, whose lanes read one position of different rows), T = 2048 / W threads a block, 41 KB for
// every tier; the loops over the widths are runtime loops over LDS rows, so nothing is indexed in registers but the accumulators.
// d_{k-1} is written over a_{k-1}: the row image of a_{k-1} is free once layer k's parameter sums have read it.
// ws: [gridDim.x][PH_MAX_LAYERS][W * W + W] doubles, per layer the weights [c_k][c_{k-1}] packed and the bias at W * W; the entries of
// a layer beyond its widths and the layers beyond ch.layers are not written.
template <int W>
__global__ __launch_bounds__(2048 / W) void patch_head_bwd_kernel(const float* __restrict__ pooled, const float* __restrict__ gy, Chain ch,
                                                                  long cells, long total, float* __restrict__ d0, double* __restrict__ ws) {
  constexpr int T = 2048 / W, NPL = W * W + W, NW = T / 64, SLOTS = (NPL + 63) / 64, ROW = T + 1, IMG = W * ROW;
  static_assert((PH_MAX_LAYERS + 1) * IMG * sizeof(float) >= NW * NPL * sizeof(double), "the wave slots reuse the images");
  __shared__ float sw[PH_MAX_LAYERS * NPL];
  __shared__ double sh[((PH_MAX_LAYERS + 1) * IMG + 1) / 2];
  float* act = reinterpret_cast<float*>(sh);         // image k < 4: a_k, image 4: d_L
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  load_chain<W, T>(ch, sw);
  const int C = ch.width[0];
  int cl = C;
#pragma unroll
  for (int k = 0; k < PH_MAX_LAYERS; ++k)
    if (k < ch.layers) cl = ch.width[k + 1];
  double acc[PH_MAX_LAYERS][SLOTS];
#pragma unroll
  for (int k = 0; k < PH_MAX_LAYERS; ++k)
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) acc[k][s] = 0.0;

  // every thread of the block takes the same number of passes (the barriers below); a thread behind the last position holds zeros
  for (long base = (long)blockIdx.x * T; base < total; base += (long)gridDim.x * T) {
    const long q = base + tid;
    const bool valid = q < total;
    const long cell = valid ? q % cells : 0, pb = valid ? q / cells : 0;
    for (int c = 0; c < C; ++c) act[c * ROW + tid] = valid ? pooled[(pb * C + c) * cells + cell] : 0.f;
    auto again = [&](auto kc) {                              // a_k from a_{k-1}, the forward's operations (layer_fwd), own column
      constexpr int k = decltype(kc)::value;
      if (k < ch.layers) {
        const int win = ch.width[k - 1], wout = ch.width[k];
        const float* wk = sw + (k - 1) * NPL;
        const float* in = act + (k - 1) * IMG + tid;
        for (int j = 0; j < wout; ++j) {
          float v = wk[W * W + j];
          for (int i = 0; i < win; ++i) v = v + wk[j * win + i] * in[i * ROW];
          act[k * IMG + j * ROW + tid] = valid ? v : 0.f;
        }
      }
    };
    again(K1{}); again(K2{}); again(K3{});
    float* d = act + PH_MAX_LAYERS * IMG;                    // the image that holds d_{k+1} when layer k (from 0) is at work
    for (int j = 0; j < cl; ++j) d[j * ROW + tid] = valid ? gy[(pb * cl + j) * cells + cell] : 0.f;
    auto back = [&](auto kc) {                               // layer k + 1 of the header comment: a_k -> a_{k+1}
      constexpr int k = decltype(kc)::value;
      if (k < ch.layers) {
        const int win = ch.width[k], wout = ch.width[k + 1], nw = wout * win;
        float* ak = act + k * IMG;
        __syncthreads();                                     // d_{k+1} and a_k of every position of the block are in place
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
          const int p = s * 64 + lane;
          if (p < nw) {
            const float* dj = d + (p / win) * ROW + wave * 64;
            const float* ai = ak + (p % win) * ROW + wave * 64;
            double t = acc[k][s];
            for (int l = 0; l < 64; ++l) t = t + (double)dj[l] * (double)ai[l];
            acc[k][s] = t;
          } else if (p < nw + wout) {
            const float* dj = d + (p - nw) * ROW + wave * 64;
            double t = acc[k][s];
            for (int l = 0; l < 64; ++l) t = t + (double)dj[l];
            acc[k][s] = t;
          }
        }
        __syncthreads();                                     // a_k has been read: d_k may take its place
        if (k > 0 || d0) {
          const float* wk = sw + k * NPL;
          for (int i = 0; i < win; ++i) {
            float v = 0.f;
            for (int j = 0; j < wout; ++j) v = v + wk[j * win + i] * d[j * ROW + tid];
            ak[i * ROW + tid] = valid ? v : 0.f;
          }
        }
        d = ak;
      }
    };
    back(K3{}); back(K2{}); back(K1{}); back(K0{});
    if (d0 && valid)
      for (int c = 0; c < C; ++c) d0[(pb * C + c) * cells + cell] = d[c * ROW + tid];
  }

  __syncthreads();                                   // the last own-column reads are done: the images become the waves' slots
  double* red = sh;                                  // [wave][NPL]
  auto slab = [&](auto kc) {
    constexpr int k = decltype(kc)::value;
    if (k < ch.layers) {
      const int nw = ch.width[k + 1] * ch.width[k], np = nw + ch.width[k + 1];
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if (s * 64 + lane < np) red[wave * NPL + s * 64 + lane] = acc[k][s];
      __syncthreads();
      for (int p = tid; p < np; p += T) {
        double t = red[p];
        for (int w = 1; w < NW; ++w) t = t + red[w * NPL + p];
        ws[((long)blockIdx.x * PH_MAX_LAYERS + k) * NPL + (p < nw ? p : W * W + (p - nw))] = t;
      }
      __syncthreads();
    }
  };
  slab(K0{}); slab(K1{}); slab(K2{}); slab(K3{});
}

// one thread per parameter: the slabs in ascending block order in float64, one rounding to fp32
__global__ __launch_bounds__(PP_THREADS) void patch_head_wgrad_finish_kernel(const double* __restrict__ ws, int slabs, int tier, Chain ch,
                                                                             ChainGrads gr) {
  const int NPL = tier * tier + tier;
  const int t0 = blockIdx.x * PP_THREADS + threadIdx.x, step = gridDim.x * PP_THREADS;
#pragma unroll
  for (int k = 0; k < PH_MAX_LAYERS; ++k) {
    if (k < ch.layers) {
      const int wout = ch.width[k + 1], nw = wout * ch.width[k];
      for (int p = t0; p < nw + wout; p += step) {
        float* dst = p < nw ? gr.w[k] : gr.b[k];
        if (!dst) continue;
        const double* src = ws + (long)k * NPL + (p < nw ? p : tier * tier + (p - nw));
        double t = 0.0;
        for (int s0 = 0; s0 < slabs; s0 += 16) {         // sixteen loads in flight, added in ascending order
          double v[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) v[u] = s0 + u < slabs ? src[(long)(s0 + u) * PH_MAX_LAYERS * NPL] : 0.0;
#pragma unroll
          for (int u = 0; u < 16; ++u)
            if (s0 + u < slabs) t = t + v[u];
        }
        dst[p < nw ? p : p - nw] = (float)t;
      }
    }
  }
}

struct Plan { Geom g; Chain ch; long positions, cells; int tier, threads, slabs; };

// false for anything the kernels do not take: the geometry's refusals, layers outside 1 .. 4, a width outside 1 .. 32, a missing weight
// among the first `layers` or a weight behind them
inline bool make_plan(int nd, int B, int C, int n0, int n1, int n2, int patch, int pool, int layers, const float* const* w, const float* const* b,
                      const int* c, Plan& pl) {
  long in_elems, out_elems;
  if (!make_geom(nd, B, C, n0, n1, n2, patch, pool, pl.g, in_elems, out_elems)) return false;
  if (layers < 1 || layers > PH_MAX_LAYERS || C > PH_MAX_WIDTH) return false;
  int wmax = C;
  pl.ch.layers = layers;
  pl.ch.width[0] = C;
  for (int k = 0; k < PH_MAX_LAYERS; ++k) {
    const bool on = k < layers;
    if (on && (c[k] < 1 || c[k] > PH_MAX_WIDTH)) return false;
    if (w && on != (w[k] != nullptr)) return false;
    pl.ch.w[k] = w && on ? w[k] : nullptr;
    pl.ch.b[k] = b && on ? b[k] : nullptr;
    pl.ch.width[k + 1] = on ? c[k] : 0;
    if (on && c[k] > wmax) wmax = c[k];
  }
  pl.tier = wmax <= 8 ? 8 : wmax <= 16 ? 16 : 32;
  pl.threads = 2048 / pl.tier;                             // of the backward: patch_head_bwd_kernel's T
  pl.positions = out_elems / C;
  pl.cells = (long)pl.g.a[0].pool * pl.g.a[1].pool * pl.g.a[2].pool;
  const long blocks = (pl.positions + pl.threads - 1) / pl.threads;
  pl.slabs = (int)(blocks > PH_BWD_MAX_BLOCKS ? PH_BWD_MAX_BLOCKS : blocks);
  return true;
}

inline unsigned fwd_blocks(long total) {
  const long b = (total + PP_THREADS - 1) / PP_THREADS;
  return (unsigned)(b > PP_MAX_BLOCKS ? PP_MAX_BLOCKS : b);
}

}  // namespace

extern "C" {
/* bytes of the float64 slab workspace of arco_patch_head_bwd / arco_patch_head_wgrad_finish; -1 for arguments they refuse */
long arco_patch_head_ws_bytes(int nd, int B, int C, int n0, int n1, int n2, int patch, int pool, int layers, int c1, int c2, int c3, int c4) {
  const int c[PH_MAX_LAYERS] = {c1, c2, c3, c4};
  Plan pl;
  if (!make_plan(nd, B, C, n0, n1, n2, patch, pool, layers, nullptr, nullptr, c, pl)) return -1;
  return (long)pl.slabs * PH_MAX_LAYERS * (pl.tier * pl.tier + pl.tier) * (long)sizeof(double);
}

int arco_patch_head_fwd(const float* x, int nd, int B, int C, int n0, int n1, int n2, int patch, int pool, int layers,
                        const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                        const float* w4, const float* b4, int c1, int c2, int c3, int c4, float* pooled, float* y, void* stream) {
  ARCO_CHECK_ARG(x && pooled && y);
  const float* w[PH_MAX_LAYERS] = {w1, w2, w3, w4};
  const float* b[PH_MAX_LAYERS] = {b1, b2, b3, b4};
  const int c[PH_MAX_LAYERS] = {c1, c2, c3, c4};
  Plan pl;
  ARCO_CHECK_ARG(make_plan(nd, B, C, n0, n1, n2, patch, pool, layers, w, b, c, pl));
  const dim3 grid(fwd_blocks(pl.positions)), block(PP_THREADS);
  if (pl.tier == 8) hipLaunchKernelGGL(patch_head_fwd_kernel<8>, grid, block, 0, as_stream(stream), x, pl.g, pl.ch, pl.positions, pooled, y);
  else if (pl.tier == 16) hipLaunchKernelGGL(patch_head_fwd_kernel<16>, grid, block, 0, as_stream(stream), x, pl.g, pl.ch, pl.positions, pooled, y);
  else hipLaunchKernelGGL(patch_head_fwd_kernel<32>, grid, block, 0, as_stream(stream), x, pl.g, pl.ch, pl.positions, pooled, y);
  return arco_launch_status();
}

/* d0 null: the gradient of the pooled tensor is not wanted (and the first layer's input gradient is not computed). */
int arco_patch_head_bwd(const float* pooled, const float* gy, int nd, int B, int C, int n0, int n1, int n2, int patch, int pool, int layers,
                        const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                        const float* w4, const float* b4, int c1, int c2, int c3, int c4, float* d0, double* ws, void* stream) {
  ARCO_CHECK_ARG(pooled && gy && ws);
  const float* w[PH_MAX_LAYERS] = {w1, w2, w3, w4};
  const float* b[PH_MAX_LAYERS] = {b1, b2, b3, b4};
  const int c[PH_MAX_LAYERS] = {c1, c2, c3, c4};
  Plan pl;
  ARCO_CHECK_ARG(make_plan(nd, B, C, n0, n1, n2, patch, pool, layers, w, b, c, pl));
  const dim3 grid(pl.slabs), block(pl.threads);
  if (pl.tier == 8)
    hipLaunchKernelGGL(patch_head_bwd_kernel<8>, grid, block, 0, as_stream(stream), pooled, gy, pl.ch, pl.cells, pl.positions, d0, ws);
  else if (pl.tier == 16)
    hipLaunchKernelGGL(patch_head_bwd_kernel<16>, grid, block, 0, as_stream(stream), pooled, gy, pl.ch, pl.cells, pl.positions, d0, ws);
  else
    hipLaunchKernelGGL(patch_head_bwd_kernel<32>, grid, block, 0, as_stream(stream), pooled, gy, pl.ch, pl.cells, pl.positions, d0, ws);
  return arco_launch_status();
}

/* gw_k [c_k, c_{k-1}], gb_k [c_k] fp32; a null pointer: that gradient is not wanted. */
int arco_patch_head_wgrad_finish(const double* ws, int nd, int B, int C, int n0, int n1, int n2, int patch, int pool, int layers,
                                 int c1, int c2, int c3, int c4, float* gw1, float* gb1, float* gw2, float* gb2, float* gw3, float* gb3,
                                 float* gw4, float* gb4, void* stream) {
  ARCO_CHECK_ARG(ws);
  const int c[PH_MAX_LAYERS] = {c1, c2, c3, c4};
  Plan pl;
  ARCO_CHECK_ARG(make_plan(nd, B, C, n0, n1, n2, patch, pool, layers, nullptr, nullptr, c, pl));
  ChainGrads gr = {{gw1, gw2, gw3, gw4}, {gb1, gb2, gb3, gb4}};
  for (int k = layers; k < PH_MAX_LAYERS; ++k) ARCO_CHECK_ARG(!gr.w[k] && !gr.b[k]);
  const int params = PH_MAX_WIDTH * PH_MAX_WIDTH + PH_MAX_WIDTH;
  hipLaunchKernelGGL(patch_head_wgrad_finish_kernel, dim3((params + PP_THREADS - 1) / PP_THREADS), dim3(PP_THREADS), 0, as_stream(stream),
                     ws, pl.slabs, pl.tier, pl.ch, gr);
  return arco_launch_status();
}
}  // extern "C"
