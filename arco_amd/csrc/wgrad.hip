// Weight gradients of the convolutions on the CDNA4 matrix cores: the kernels, the fixed-order slab reductions, the route
// (wgrad_plan: pure host code, shared by the launch and the query arco_wgrad_config), the launch, and the column sums of
// the bias gradient.  The f16-storage kernels of the family live in conv_h.hip and are launched through the same plan.
#include "wgrad.h"
#include "split_bf16.h"
#include <stdlib.h>

// ---------------------------------------------------------------------------
// weight gradient:  dW[co][ci][tap] = sum_pix dZ[pix][co] * Ain[pix + tap][ci]
// M = co, N = ci, K = pixels.  grid.x = pixel chunk, grid.y = co tile,
// grid.z = tap * ci_tiles + ci tile.  Tiles of 128 pixels (8x16) are staged channels-last in
// LDS (row stride = 16 mod 32 dwords -> conflict-free ds_read_b32 of 16 channels x 4
// pixels); each wave reduces 32 pixels per tile; partial slabs are summed in fixed
// order by wgrad_reduce_kernel (deterministic).
// ---------------------------------------------------------------------------
// ablation bits of tools/micro/wgrad_abl.py / wgrad1_bench.py: compiled in only with -DARCO_WGRAD_ABLATION (as run-time
// branches they cost wgrad_split_kernel<16,16> 8 VGPRs and 56 % of its speed)
#ifdef ARCO_WGRAD_ABLATION
#define WGRAD_ABL(a) ((a).abl)
#else
#define WGRAD_ABL(a) 0
#endif
struct WgradArgs {
  const float* dZ; long ldz; int Cout;
  const float* Ain; long lda; int Cin;
  int taps, NB, H, W, D3; long M;
  float* partial;      // [chunks][taps][CoutPad][CinPad]
  int CoutPad, CinPad, n_tiles;
  int mma;             // 0 fp32 MFMA; 2: bf16 operands (halo kernels, 3x3x3 only), fp32 accumulate
  int abl;             // ablation bits for tools/micro/wgrad_abl.py (0 in the product): 1 no MFMA phase, 2 no staging, 4 no global loads
  ArcoActPro pro;      // pro.mean != nullptr: Ain holds the pre-activation z of the producing conv; the loader applies BN + LeakyReLU + dropout
                       // (wgrad_split_kernel, 3x3: the weight gradient of a block's second convolution reads z1, not a stored activation)
};

constexpr int WGRAD1_PAD = 8;
template <int CO_B, int CI_B>
__global__ __launch_bounds__(256) void wgrad_kernel(WgradArgs a) {
  // row pad 8 (was 16): 64 x 64 blocks take 73.7 KB instead of 82 KB of LDS - TWO workgroups per CU, so one stages while the
  // other is on the matrix cores (the staging loads are not prefetched); the fragment reads become 2-way bank conflicts,
  // 8 reads against 16 MFMAs per K step
  constexpr int LDZ = (CO_B % 32 == 0) ? CO_B + WGRAD1_PAD : CO_B;
  constexpr int LDA = (CI_B % 32 == 0) ? CI_B + WGRAD1_PAD : CI_B;
  constexpr int CO_T = CO_B / 16, CI_T = CI_B / 16;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Zs = smem;                 // [128][LDZ]
  float* Xs = smem + 128 * LDZ;     // [128][LDA]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
  const int ci_tiles = a.CinPad / CI_B;
  const int tap = blockIdx.z / ci_tiles, cit = blockIdx.z % ci_tiles;
  const int co0 = blockIdx.y * CO_B, ci0 = cit * CI_B;
  const bool sp = a.taps >= 9;                     // spatial taps (3x3 per plane, x3 planes when taps == 27)
  const int t9 = tap % 9, dpl = a.taps == 27 ? tap / 9 - 1 : 0;
  const int dy = sp ? t9 / 3 - 1 : 0, dx = sp ? t9 % 3 - 1 : 0;
  const int tiles_x = (a.W + 15) / 16, tiles_y = (a.H + 7) / 8;

  f32x4 acc[CO_T][CI_T];
#pragma unroll
  for (int i = 0; i < CO_T; ++i)
#pragma unroll
    for (int j = 0; j < CI_T; ++j) acc[i][j] = f32x4{0, 0, 0, 0};

  // the next tile's operands travel global -> registers while this tile is on the matrix cores (fetch), registers -> LDS
  // behind the barrier (stage): unprefetched staging loads were 100 of the 180 us of the 16 384 x 448 x 448 head gradient
  constexpr int NZ = 128 * (CO_B / 4) / 256, NX = 128 * (CI_B / 4) / 256;
  f32x4 rz[NZ], rx[NX];
  auto fetch = [&](int t) {
    int img = 0, y0 = 0, x0 = 0; long m0 = 0;
    if (sp) {
      int tt = t; const int tx = tt % tiles_x; tt /= tiles_x; const int ty = tt % tiles_y; img = tt / tiles_y;
      y0 = ty * 8; x0 = tx * 16;
    } else {
      m0 = (long)t * 128;
    }
#pragma unroll
    for (int it = 0; it < NZ; ++it) {
      const int idx = tid + it * 256;
      const int p = idx / (CO_B / 4), q = idx % (CO_B / 4);
      long pix = -1;
      if (sp) { const int y = y0 + p / 16, x = x0 + p % 16; if (y < a.H && x < a.W) pix = ((long)img * a.H + y) * a.W + x; }
      else { const long m = m0 + p; if (m < a.M) pix = m; }
      f32x4 v = f32x4{0, 0, 0, 0};
      if (pix >= 0) {
        const int c = co0 + 4 * q;
        const float* src = a.dZ + pix * a.ldz + c;
        if (((a.Cout & 3) == 0) && ((a.ldz & 3) == 0)) { if (c < a.Cout) v = *reinterpret_cast<const f32x4*>(src); }
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (c + e < a.Cout) v[e] = src[e];
        }
      }
      rz[it] = v;
    }
#pragma unroll
    for (int it = 0; it < NX; ++it) {
      const int idx = tid + it * 256;
      const int p = idx / (CI_B / 4), q = idx % (CI_B / 4);
      long pix = -1;
      if (sp) {
        const int yo = y0 + p / 16, xo = x0 + p % 16;
        const int y = yo + dy, x = xo + dx;
        const int pl = a.taps == 27 ? img % a.D3 + dpl : 0;
        if (yo < a.H && xo < a.W && y >= 0 && y < a.H && x >= 0 && x < a.W && pl >= 0 && pl < a.D3)
          pix = ((long)(img + dpl) * a.H + y) * a.W + x;
      } else { const long m = m0 + p; if (m < a.M) pix = m; }
      f32x4 v = f32x4{0, 0, 0, 0};
      if (pix >= 0) {
        const int c = ci0 + 4 * q;
        const float* src = a.Ain + pix * a.lda + c;
        if (((a.Cin & 3) == 0) && ((a.lda & 3) == 0)) { if (c < a.Cin) v = *reinterpret_cast<const f32x4*>(src); }
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (c + e < a.Cin) v[e] = src[e];
        }
      }
      rx[it] = v;
    }
  };
  int t = blockIdx.x;
  if (t < a.n_tiles) fetch(t);
  for (; t < a.n_tiles; t += gridDim.x) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < NZ; ++it) {
      const int idx = tid + it * 256;
      *reinterpret_cast<f32x4*>(&Zs[(idx / (CO_B / 4)) * LDZ + 4 * (idx % (CO_B / 4))]) = rz[it];
    }
#pragma unroll
    for (int it = 0; it < NX; ++it) {
      const int idx = tid + it * 256;
      *reinterpret_cast<f32x4*>(&Xs[(idx / (CI_B / 4)) * LDA + 4 * (idx % (CI_B / 4))]) = rx[it];
    }
    __syncthreads();
    if (t + (int)gridDim.x < a.n_tiles) fetch(t + gridDim.x);
    const int pw = wid * 32;
#pragma unroll 4
    for (int ks = 0; ks < 8; ++ks) {
      const int p = pw + ks * 4 + g;
      float zf[CO_T], xf[CI_T];
#pragma unroll
      for (int i = 0; i < CO_T; ++i) zf[i] = Zs[p * LDZ + i * 16 + li];
#pragma unroll
      for (int j = 0; j < CI_T; ++j) xf[j] = Xs[p * LDA + j * 16 + li];
#pragma unroll
      for (int i = 0; i < CO_T; ++i)
#pragma unroll
        for (int j = 0; j < CI_T; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(zf[i], xf[j], acc[i][j], 0, 0, 0);
    }
  }
  // cross-wave reduction through LDS, then slab store
  __syncthreads();
  float* red = smem;   // [4][CO_B][CI_B]
#pragma unroll
  for (int i = 0; i < CO_T; ++i)
#pragma unroll
    for (int j = 0; j < CI_T; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        red[((wid * CO_B) + i * 16 + 4 * g + r) * CI_B + j * 16 + li] = acc[i][j][r];
  __syncthreads();
  float* out = a.partial + (((long)blockIdx.x * a.taps + tap) * a.CoutPad) * a.CinPad;
  for (int idx = tid; idx < CO_B * CI_B; idx += 256) {
    const int co = idx / CI_B, ci = idx % CI_B;
    const float v = (red[(0 * CO_B + co) * CI_B + ci] + red[(1 * CO_B + co) * CI_B + ci]) +
                    (red[(2 * CO_B + co) * CI_B + ci] + red[(3 * CO_B + co) * CI_B + ci]);
    out[(long)(co0 + co) * a.CinPad + ci0 + ci] = v;
  }
}

// ---------------------------------------------------------------------------
// 1x1 weight gradient of the WIDE heads (FeatureExtractor fea3 / fea4, q_representation: model_2D.py:46-53, train_arco_2d.py:231-234;
// dW [496 x 496] = dY^T [496 x M] . X [M x 496] at M = 5 x 10^5): 128 x 128 output blocks, each WAVE owns a 64 x 64 quadrant for
// all 128 pixels of a tile.  wgrad_kernel<64,64> gives every wave the whole 64 x 64 block for a quarter of the pixels: its
// 8 x 8 = 64 blocks read each operand eight times (16.6 GB at M = 524 288: 53 TFLOP/s, bound by L2 / HBM traffic); here 4 x 4
// blocks read each operand four times, no cross-wave reduction, one workgroup per CU (139 KB of LDS), the next tile's 128 KB
// travelling global -> registers under the current tile's 512 fp32 MFMAs per wave.  Same products and per-block summation
// order over pixels as wgrad_kernel within a slab; slabs are summed in fixed order by wgrad_reduce_kernel.
// ---------------------------------------------------------------------------
template <int TP>       // pixels per staged tile: 64 (70 KB of LDS, two workgroups per CU; 128 needed 139 KB, one per CU, and was retired)
__global__ __launch_bounds__(256) void wgrad_q_kernel(WgradArgs a) {
  constexpr int CO_B = 128, CI_B = 128, LDZ = CO_B + WGRAD1_PAD, LDA = CI_B + WGRAD1_PAD;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Zs = smem;                 // [TP][LDZ]
  float* Xs = smem + TP * LDZ;      // [TP][LDA]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
  const int wr = wid >> 1, wc = wid & 1;
  const int co0 = blockIdx.y * CO_B, ci0 = blockIdx.z * CI_B;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0, 0, 0, 0};
  constexpr int NP = TP * (128 / 4) / 256;           // 16-byte pieces per thread, tile and operand (16 / 8)
  f32x4 rz[NP], rx[NP];
  auto fetch = [&](int t) {
    const long m0 = (long)t * TP;
#pragma unroll
    for (int it = 0; it < NP; ++it) {
      const int idx = tid + it * 256, p = idx >> 5, q = idx & 31;
      const long m = m0 + p;
      const int cz = co0 + 4 * q, cx = ci0 + 4 * q;
      // clamped addresses + a select: branch-free loads (a conditional load puts a vmcnt(0) behind every piece)
      const bool okz = m < a.M && cz < a.Cout, okx = m < a.M && cx < a.Cin;
      const f32x4 vz = *reinterpret_cast<const f32x4*>(okz ? a.dZ + m * a.ldz + cz : a.dZ);
      const f32x4 vx = *reinterpret_cast<const f32x4*>(okx ? a.Ain + m * a.lda + cx : a.Ain);
      rz[it] = okz ? vz : f32x4{0, 0, 0, 0};
      rx[it] = okx ? vx : f32x4{0, 0, 0, 0};
    }
  };
  int t = blockIdx.x;
  if (t < a.n_tiles) fetch(t);
  for (; t < a.n_tiles; t += gridDim.x) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < NP; ++it) {
      const int idx = tid + it * 256, p = idx >> 5, q = idx & 31;
      *reinterpret_cast<f32x4*>(&Zs[p * LDZ + 4 * q]) = rz[it];
      *reinterpret_cast<f32x4*>(&Xs[p * LDA + 4 * q]) = rx[it];
    }
    __syncthreads();
    if (t + (int)gridDim.x < a.n_tiles) fetch(t + gridDim.x);
#pragma unroll 4
    for (int ks = 0; ks < TP / 4; ++ks) {
      const int p = ks * 4 + g;
      float zf[4], xf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) zf[i] = Zs[p * LDZ + (wr * 4 + i) * 16 + li];
#pragma unroll
      for (int j = 0; j < 4; ++j) xf[j] = Xs[p * LDA + (wc * 4 + j) * 16 + li];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(zf[i], xf[j], acc[i][j], 0, 0, 0);
    }
  }
  float* out = a.partial + ((long)blockIdx.x * a.CoutPad) * a.CinPad;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(long)(co0 + (wr * 4 + i) * 16 + 4 * g + r) * a.CinPad + ci0 + (wc * 4 + j) * 16 + li] = acc[i][j][r];
}

// ---------------------------------------------------------------------------
// all-taps weight gradient for the shallow layers (Cout, Cin <= 32): one block owns a tile of 8x16 output
// pixels of one plane, stages the dZ tile and the input HALO patch once in LDS and accumulates all 9 taps of
// the plane (3-D: the depth tap dd = blockIdx.z, input plane x+dd-1) -> both operands are read from HBM/L2
// once instead of once per tap.  The A fragment (dZ^T) is shared by the 9 taps.
// partial layout identical to wgrad_kernel: [chunk][tap][CoutPad][CinPad].
// ---------------------------------------------------------------------------
// Persistent over pixel tiles with the NEXT tile's operands prefetched into
// registers during the MFMAs.  The block's CO_B x CI_B outputs are split into 16x16 sub-tiles; each sub-tile is
// owned by 4 / n_sub waves for all 9 taps (32x32: one wave per sub-tile walking all 128 pixels -> no cross-wave
// reduction, 36 accumulator registers instead of 144; 16x32 / 32x16: two waves per sub-tile, 64 pixels each;
// 16x16: four waves, 32 pixels each), partners are summed once per LAUNCH through LDS.
// FLAT: tiles are 128 consecutive positions of the plane stored with padded row stride W + 2 (see igemm_kernel FLAT)
// MMA = 2: 16 pixels per step instead of 4 - a lane converts 4 consecutive pixels of dZ and of each tap's input
// to bf16 and issues one v_mfma_f32_16x16x16_bf16 per tap (see igemm_kernel's MMA note; gradients use bf16, not f16:
// dZ values of 1e-6 would flush in f16).
template <int CO_B, int CI_B, bool FLAT = false, int MMA = 0>
__global__ __launch_bounds__(256) void wgrad_halo2_kernel(WgradArgs a) {
  constexpr int LDZ = (CO_B % 32 == 0) ? CO_B + 16 : CO_B;
  constexpr int LDA = (CI_B % 32 == 0) ? CI_B + 16 : CI_B;
  constexpr int QZ = CO_B / 4, QA = CI_B / 4, HROWS = FLAT ? 128 + 2 * IGEMM_FLAT_WPMAX + 2 : 10 * 18;
  constexpr int NZ = (128 * QZ + 255) / 256, NX = (HROWS * QA + 255) / 256;
  constexpr int CI_T = CI_B / 16, NSUB = (CO_B / 16) * CI_T, WPS = 4 / NSUB, KSTEPS = 32 / WPS;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Zs = smem;                 // [128][LDZ]
  float* Xs = smem + 128 * LDZ;     // [180][LDA]   halo patch
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
  const int sub = wid / WPS, part = wid % WPS, wi = sub / CI_T, wj = sub % CI_T;
  const int dd = blockIdx.z;                                   // depth tap (3-D) ; 0 for 2-D
  const int dpl = a.taps == 27 ? dd - 1 : 0;
  const int tiles_x = (a.W + 15) / 16, tiles_y = (a.H + 7) / 8;
  const int Wp = a.W + 2, flat_per_plane = (a.H * Wp + 127) / 128;
  const int ci_tiles = a.CinPad / CI_B;
  const int co0 = (blockIdx.y / ci_tiles) * CO_B, ci0 = (blockIdx.y % ci_tiles) * CI_B;
  const bool vz = ((a.Cout & 3) == 0) && ((a.ldz & 3) == 0), vx = ((a.Cin & 3) == 0) && ((a.lda & 3) == 0);

  f32x4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = f32x4{0, 0, 0, 0};
  f32x4 pz[NZ], px_[NX];
  auto fetch = [&](int t) {
    int tt = t; const int tx = tt % tiles_x; tt /= tiles_x; const int ty = tt % tiles_y;
    const int img = FLAT ? t / flat_per_plane : tt / tiles_y;
    const int y0 = ty * 8, x0 = tx * 16, f0 = FLAT ? (t - img * flat_per_plane) * 128 : 0;
    const int pl = a.taps == 27 ? img % a.D3 + dpl : 0;
    const bool plane_ok = pl >= 0 && pl < a.D3;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
      const int idx = tid + i * 256, p = idx / QZ, q = idx % QZ;
      const int fy = (f0 + p) / Wp, fx = (f0 + p) - fy * Wp;                  // FLAT: output position -> (row, padded column)
      const int y = FLAT ? fy : y0 + p / 16, x = FLAT ? fx - 1 : x0 + p % 16, c = co0 + 4 * q;
      f32x4 v = f32x4{0, 0, 0, 0};
      if (idx < 128 * QZ && y < a.H && x >= 0 && x < a.W && plane_ok) {
        const float* src = a.dZ + (((long)img * a.H + y) * a.W + x) * a.ldz + c;
        if (vz) { if (c < a.Cout) v = *reinterpret_cast<const f32x4*>(src); }
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (c + e < a.Cout) v[e] = src[e];
        }
      }
      pz[i] = v;
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int idx = tid + i * 256, r = idx / QA, q = idx % QA;
      const int pidx = f0 + r - 1, py = pidx >= 0 ? pidx / Wp : -1, ppx = pidx - py * Wp;      // FLAT: padded-plane position
      const int y = FLAT ? py - 1 : y0 + r / 18 - 1, x = FLAT ? ppx - 1 : x0 + r % 18 - 1, c = ci0 + 4 * q;
      f32x4 v = f32x4{0, 0, 0, 0};
      if (idx < HROWS * QA && (!FLAT || (pidx >= 0 && r < 128 + 2 * Wp + 2)) && y >= 0 && y < a.H && x >= 0 && x < a.W && plane_ok) {
        const float* src = a.Ain + (((long)(img + dpl) * a.H + y) * a.W + x) * a.lda + c;
        if (vx) { if (c < a.Cin) v = *reinterpret_cast<const f32x4*>(src); }
        else {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (c + e < a.Cin) v[e] = src[e];
        }
      }
      px_[i] = v;
    }
  };

  int t = blockIdx.x;
  if (t < a.n_tiles) fetch(t);
  while (t < a.n_tiles) {
#pragma unroll
    for (int i = 0; i < NZ; ++i) { const int idx = tid + i * 256; if (idx < 128 * QZ) *reinterpret_cast<f32x4*>(&Zs[(idx / QZ) * LDZ + 4 * (idx % QZ)]) = pz[i]; }
#pragma unroll
    for (int i = 0; i < NX; ++i) { const int idx = tid + i * 256; if (idx < HROWS * QA) *reinterpret_cast<f32x4*>(&Xs[(idx / QA) * LDA + 4 * (idx % QA)]) = px_[i]; }
    __syncthreads();
    const int next = t + gridDim.x;
    if (next < a.n_tiles) fetch(next);
    if constexpr (MMA == 2) {
#pragma unroll 2
      for (int k4 = 0; k4 < KSTEPS / 4; ++k4) {
        const int p0 = (part * KSTEPS + 4 * k4) * 4 + 4 * g, py = p0 >> 4, pxx = p0 & 15;   // pixels p0 .. p0+3: one tile row
        f32x4 zv;
#pragma unroll
        for (int j = 0; j < 4; ++j) zv[j] = Zs[(p0 + j) * LDZ + wi * 16 + li];
        const s16x4 zh = to_bf16x4(zv);
        const float* xrow = Xs + (FLAT ? p0 : py * 18 + pxx) * LDA + wj * 16 + li;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int toff = (FLAT ? (tap / 3) * Wp + tap % 3 : (tap / 3) * 18 + tap % 3) * LDA;
          f32x4 xv;
#pragma unroll
          for (int j = 0; j < 4; ++j) xv[j] = xrow[toff + j * LDA];
          acc[tap] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(zh, to_bf16x4(xv), acc[tap], 0, 0, 0);
        }
      }
    } else {
#pragma unroll 4
    for (int ks = 0; ks < KSTEPS; ++ks) {
      const int p = (part * KSTEPS + ks) * 4 + g, py = p >> 4, pxx = p & 15;
      const float zf = Zs[p * LDZ + wi * 16 + li];
      const float* xrow = Xs + (FLAT ? p : py * 18 + pxx) * LDA + wj * 16 + li;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        acc[tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(zf, xrow[(FLAT ? (tap / 3) * Wp + tap % 3 : (tap / 3) * 18 + tap % 3) * LDA], acc[tap], 0, 0, 0);
    }
    }
    __syncthreads();
    t = next;
  }
  if (WPS > 1) {                      // sum the pixel-split partner waves (once per launch)
    float* red = smem;                // [4 waves][9][256]
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wid * 9 + tap) * 256 + r * 64 + lane] = acc[tap][r];
    __syncthreads();
    if (part == 0) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[tap][r];
#pragma unroll
          for (int w2 = 1; w2 < WPS; ++w2) v += red[((wid + w2) * 9 + tap) * 256 + r * 64 + lane];
          acc[tap][r] = v;
        }
    }
  }
  if (part == 0) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      float* out = a.partial + (((long)blockIdx.x * a.taps + dd * 9 + tap) * a.CoutPad) * a.CinPad;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(long)(co0 + wi * 16 + 4 * g + r) * a.CinPad + ci0 + wj * 16 + li] = acc[tap][r];
    }
  }
}

// ---------------------------------------------------------------------------
// Split-bf16 weight gradient of the 3x3 / 3x3x3 convolutions (the MMA = 3 counterpart of wgrad_halo2_kernel):
//   dW[tap][co][ci] = sum_pix dZ[pix][co] * X[pix + tap][ci],   M = co, N = ci, K = PIXELS.
// v_mfma_f32_16x16x32_bf16 wants 8 consecutive k (= pixels) per lane, so both operands are staged TRANSPOSED in LDS, as
// three bf16 planes [plane][channel][pixel]: a staging thread loads 4 consecutive pixels x 4 channels (four 16-byte global
// loads), splits every value into its three bf16 terms and writes, per channel and plane, the 4 pixels as one 8-byte word.
// One K step = 32 pixels = two rows of the 8 x 16 tile; lane (li, g) supplies channel li, row 2s + (g >> 1), columns
// 8 (g & 1) .. + 7.  The input operand of tap (dy, dx) is the halo tile shifted by dx columns: a lane reads the 12 columns
// 8h .. 8h + 11 of row r + dy once (ds_read_b128 + ds_read_b64) and forms the three dx windows in registers (dx = 1: four
// v_alignbit_b32, dx = 2: the next dwords) - 18 LDS reads feed the 54 MFMAs of a K step.  Persistent over tiles with the
// next tile's global loads in flight during the MFMAs; partial layout / reduction identical to wgrad_halo2_kernel.
// ---------------------------------------------------------------------------
// LDS channel rows of wgrad_split_kernel.  PMC (tools/pmc_lds_step.sh): with plain rows of 68 / 124 dwords TWO THIRDS of the kernel's
// LDS cycles were bank conflicts - the staging stores (8 lanes = 8 channel quads of one pixel group, channel stride 4 rows = 16 mod 32
// banks: 4-way) and the fragment reads (2-way).  The dword offset inside a channel's row is XOR-ed with 4 * (channel / 4): the eight
// quads of a store group land in eight different 4-dword blocks, and with rows of 72 / 136 dwords the ds_read_b128 groups are
// conflict-free as well (model: tools/micro/lds_bank_model.py - stores 4 -> 1.0 / 1.2, b128 reads 2 -> 1.0 / 1.5 cycles per group).
// (WG_SWZ = false with rows of 68 / 124 is round 2's layout.)
constexpr bool WG_SWZ = true;
constexpr int WG_CSZ = WG_SWZ ? 72 : 68;
constexpr int WG_CSX = WG_SWZ ? 136 : 124;
template <int CO_B, int CI_B, bool PRO = false>
__global__ __launch_bounds__(256) void wgrad_split_kernel(WgradArgs a) {
  constexpr int QZ = CO_B / 4, QA = CI_B / 4;
  constexpr int ZU = 32 * QZ, XU = 50 * QA;                 // staging units (4 pixels x 4 channels)
  constexpr int NZU = (ZU + 255) / 256, NXU = (XU + 255) / 256;
  constexpr int CSZ = WG_CSZ, CSX = WG_CSX;      // dwords per (plane, channel) row: 128 px / 10 x 24 halo px (+ pad)
  constexpr int CI_T = CI_B / 16, NSUB = (CO_B / 16) * CI_T, WPS = 4 / NSUB, KS = 4 / WPS;
  extern __shared__ __attribute__((aligned(16))) unsigned int smem_u[];
  unsigned int* Zs = smem_u;                                // [3][CO_B][CSZ]
  unsigned int* Xs = smem_u + 3 * CO_B * CSZ;               // [3][CI_B][CSX]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 15, g = lane >> 4;
  const int sub = wid / WPS, part = wid % WPS, wi = sub / CI_T, wj = sub % CI_T;
  const int dd = blockIdx.z;
  const int dpl = a.taps == 27 ? dd - 1 : 0;
  const int tiles_x = (a.W + 15) / 16, tiles_y = (a.H + 7) / 8;
  const int ci_tiles = a.CinPad / CI_B;
  const int co0 = (blockIdx.y / ci_tiles) * CO_B, ci0 = (blockIdx.y % ci_tiles) * CI_B;

  f32x4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = f32x4{0, 0, 0, 0};
  f32x4 pz[NZU][4], px_[NXU][4];
  // consumer-side activation of the input operand (PRO): pixel origin of the fetched tile, the parameter quads of
  // this thread's channels for the BatchNorm group of the tile being staged (reloaded when the group changes: at most once per launch
  // and workgroup - tiles are walked in image order)
  int f_img = 0, f_y0 = 0, f_x0 = 0, pgrp = -1;
  ProQuad pq[NXU];
  const int ipg = PRO ? a.NB / (a.pro.groups > 1 ? a.pro.groups : 1) : 1;
  const bool pdrop = PRO && a.pro.drop_mode == 1;
  uint32_t dkey = 0, dthr = 0; float keep_scale = 1.f;
  if (PRO && pdrop) {
    const unsigned long long sd = a.pro.seed_dev ? a.pro.seed ^ (a.pro.seed_dev[0] * 0x9E3779B97F4A7C15ull) : a.pro.seed;
    dkey = drop_key32(sd); dthr = drop_thr16(a.pro.p); keep_scale = 1.0f / (1.0f - a.pro.p);
  }
  auto fetch = [&](int t) {
    int tt = t; const int tx = tt % tiles_x; tt /= tiles_x; const int ty = tt % tiles_y; const int img = tt / tiles_y;
    const int y0 = ty * 8, x0 = tx * 16;
    if (PRO) { f_img = img; f_y0 = y0; f_x0 = x0; }
    const int pl = a.taps == 27 ? img % a.D3 + dpl : 0;
    const bool plane_ok = pl >= 0 && pl < a.D3;
#pragma unroll
    for (int i = 0; i < NZU; ++i) {
      const int u = tid + i * 256, pg = u / QZ, q = u % QZ, r = pg >> 2, cg = pg & 3;
      const int y = y0 + r, c = co0 + 4 * q;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = x0 + 4 * cg + j;
        f32x4 v = f32x4{0, 0, 0, 0};
        if (u < ZU && y < a.H && x < a.W && plane_ok && c < a.Cout) v = *reinterpret_cast<const f32x4*>(a.dZ + (((long)img * a.H + y) * a.W + x) * a.ldz + c);
        pz[i][j] = v;
      }
    }
#pragma unroll
    for (int i = 0; i < NXU; ++i) {
      const int u = tid + i * 256, pg = u / QA, q = u % QA, hr = pg / 5, hg = pg % 5;
      const int y = y0 + hr - 1, c = ci0 + 4 * q;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = x0 - 1 + 4 * hg + j;
        f32x4 v = f32x4{0, 0, 0, 0};
        if (u < XU && y >= 0 && y < a.H && x >= 0 && x < a.W && plane_ok && c < a.Cin) {
          v = *reinterpret_cast<const f32x4*>(a.Ain + (((long)(img + dpl) * a.H + y) * a.W + x) * a.lda + c);
        }
        px_[i][j] = v;
      }
    }
  };
  // 4 pixels x 4 channels -> per channel and plane one 8-byte word of 4 bf16 pixels
  auto stage = [&](const f32x4 (&v)[4], unsigned int* base, int nchan, int chan0, int cs, int off) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      u32x2 p0, p1, p2;
      split3_bf16x4(f32x4{v[0][e], v[1][e], v[2][e], v[3][e]}, p0, p1, p2);
      unsigned int* d = base + (long)(chan0 + e) * cs + (WG_SWZ ? (off ^ (((chan0 >> 2) & 7) << 2)) : off);
      *reinterpret_cast<u32x2_ma*>(d) = p0;
      *reinterpret_cast<u32x2_ma*>(d + (long)nchan * cs) = p1;
      *reinterpret_cast<u32x2_ma*>(d + 2l * nchan * cs) = p2;
    }
  };

  const int swz_z = WG_SWZ ? (((wi * 16 + li) >> 2) & 7) << 2 : 0, swz_x = WG_SWZ ? (((wj * 16 + li) >> 2) & 7) << 2 : 0;
  int t = blockIdx.x;
  if (t < a.n_tiles && !(WGRAD_ABL(a) & 4)) fetch(t);
  while (t < a.n_tiles) {
    if (!(WGRAD_ABL(a) & 2)) {
#pragma unroll
    for (int i = 0; i < NZU; ++i) {
      const int u = tid + i * 256, pg = u / QZ, q = u % QZ, r = pg >> 2, cg = pg & 3;
      if (u < ZU) stage(pz[i], Zs, CO_B, 4 * q, CSZ, r * 8 + cg * 2);
    }
    if constexpr (PRO) {        // a = dropout(lrelu(BN(z))) on the fetched quads (zero padding stays zero), as bn_act_fwd_kernel computes it
      const int grp = f_img / ipg;
      if (grp != pgrp) {
        pgrp = grp;
#pragma unroll
        for (int i = 0; i < NXU; ++i) {
          const int u = tid + i * 256, q = u % QA;
          int c = ci0 + 4 * q; if (c + 4 > a.Cin) c = 0;
          pq[i].mu = *reinterpret_cast<const f32x4*>(a.pro.mean + (long)grp * a.Cin + c);
          pq[i].is = *reinterpret_cast<const f32x4*>(a.pro.istd + (long)grp * a.Cin + c);
          pq[i].ga = *reinterpret_cast<const f32x4*>(a.pro.gamma + c);
          pq[i].be = *reinterpret_cast<const f32x4*>(a.pro.beta + c);
        }
      }
      // Tiles whose halo lies inside the image (all but the image's border ring) need no zeroing: the arithmetic alone costs next to
      // nothing, arithmetic + per-pixel zeroing 40 us on the 16 -> 16 layer at 256^2 (tools/micro/wgrad_pro_bench.py) - wave-uniform branch
      const bool interior = f_y0 > 0 && f_y0 + 9 <= a.H && f_x0 > 0 && f_x0 + 17 <= a.W && (a.Cin % CI_B) == 0;
      if (interior) {
#pragma unroll
        for (int i = 0; i < NXU; ++i) {
          const int u = tid + i * 256, pg = u / QA, q = u % QA, hr = pg / 5, hg = pg % 5;
          const uint32_t e0 = (uint32_t)(((f_img * a.H + f_y0 + hr - 1) * a.W + f_x0 - 1 + 4 * hg) * a.Cin + ci0 + 4 * q);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            f32x4 v = pro_bn_lrelu(px_[i][j], pq[i], a.pro.slope);
            if (pdrop) v = pro_dropout(v, dkey, e0 + (uint32_t)(j * a.Cin), dthr, keep_scale);
            px_[i][j] = v;
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < NXU; ++i) {
          const int u = tid + i * 256, pg = u / QA, q = u % QA, hr = pg / 5, hg = pg % 5;
          const uint32_t e0 = (uint32_t)(((f_img * a.H + f_y0 + hr - 1) * a.W + f_x0 - 1 + 4 * hg) * a.Cin + ci0 + 4 * q);
          const int y = f_y0 + hr - 1;
          const bool rok = u < XU && y >= 0 && y < a.H && ci0 + 4 * q < a.Cin;      // (validity recomputed here, on border tiles only: no mask carried from fetch)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int x = f_x0 - 1 + 4 * hg + j;
            f32x4 v = pro_bn_lrelu(px_[i][j], pq[i], a.pro.slope);
            if (pdrop) v = pro_dropout(v, dkey, e0 + (uint32_t)(j * a.Cin), dthr, keep_scale);
            px_[i][j] = pro_mask(v, (rok && x >= 0 && x < a.W) ? 1u : 0u);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NXU; ++i) {
      const int u = tid + i * 256, pg = u / QA, q = u % QA, hr = pg / 5, hg = pg % 5;
      if (u < XU) stage(px_[i], Xs, CI_B, 4 * q, CSX, hr * 12 + hg * 2);
    }
    }
    __syncthreads();
    const int next = t + gridDim.x;
    if (next < a.n_tiles && !(WGRAD_ABL(a) & 4)) fetch(next);
    if (!(WGRAD_ABL(a) & 1))
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int s = part * KS + ks, rr = 2 * s + (g >> 1), h = g & 1;
      bf16x8 za[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) za[p] = lds_bf16x8(&Zs[(p * CO_B + wi * 16 + li) * CSZ + ((rr * 8 + h * 4) ^ swz_z)]);
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        unsigned int w[3][6];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          const unsigned int* row = &Xs[(p * CI_B + wj * 16 + li) * CSX];
          const int o = (rr + dy) * 12 + h * 4;
          const u32x4 lo = *reinterpret_cast<const u32x4_ma*>(row + (o ^ swz_x));
          const u32x2 hi = *reinterpret_cast<const u32x2_ma*>(row + ((o + 4) ^ swz_x));
          w[p][0] = lo[0]; w[p][1] = lo[1]; w[p][2] = lo[2]; w[p][3] = lo[3];
          w[p][4] = hi[0]; w[p][5] = hi[1];
        }
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          bf16x8 xb[3];
#pragma unroll
          for (int p = 0; p < 3; ++p) {
            unsigned int d4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
              d4[i] = dx == 0 ? w[p][i] : (dx == 2 ? w[p][i + 1] : __builtin_amdgcn_alignbit(w[p][i + 1], w[p][i], 16));
            xb[p] = __builtin_bit_cast(bf16x8, u32x4{d4[0], d4[1], d4[2], d4[3]});
          }
          f32x4 c = acc[dy * 3 + dx];
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(za[2], xb[0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(za[0], xb[2], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(za[1], xb[1], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(za[1], xb[0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(za[0], xb[1], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(za[0], xb[0], c, 0, 0, 0);
          acc[dy * 3 + dx] = c;
        }
      }
    }
    __syncthreads();
    t = next;
  }
  if (WPS > 1) {                      // sum the pixel-split partner waves (once per launch)
    float* red = reinterpret_cast<float*>(smem_u);                // [4 waves][9][256]
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wid * 9 + tap) * 256 + r * 64 + lane] = acc[tap][r];
    __syncthreads();
    if (part == 0) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[tap][r];
#pragma unroll
          for (int w2 = 1; w2 < WPS; ++w2) v += red[((wid + w2) * 9 + tap) * 256 + r * 64 + lane];
          acc[tap][r] = v;
        }
    }
  }
  if (part == 0) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      float* out = a.partial + (((long)blockIdx.x * a.taps + dd * 9 + tap) * a.CoutPad) * a.CinPad;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(long)(co0 + wi * 16 + 4 * g + r) * a.CinPad + ci0 + wj * 16 + li] = acc[tap][r];
    }
  }
}

// Weight gradient of the one-channel 3x3x3 layer: dW[co][tap] = sum_vox dZ[vox][co] * X[vox + tap].
// D[tap][co] = im2col^T [tap][vox] * dZ [vox][co]: M = 27 taps (two 16-row MFMA tiles), N = 16, K = voxels; the im2col
// operand comes from a three-plane halo tile in LDS, dZ is read once straight from HBM (64 B per voxel, coalesced).
// Persistent over 16 x 16 tiles; the four waves split a tile's voxels; one slab [27][CoutPad][CinPad] per workgroup
// in the layout of the generic kernels (only ci = 0 is used) -> wgrad_reduce_kernel finishes.
// DEPTH = 1: one-channel image, 9 taps (one MFMA tile of taps).
template <int DEPTH>
__global__ __launch_bounds__(256) void wgrad_image3d_kernel(WgradArgs a) {
  constexpr int TH = 16, TW = 16, HW_ = TW + 2, NP = (TH + 2) * HW_, NT = 9 * DEPTH;
  __shared__ float Xs[DEPTH * NP];
  __shared__ __attribute__((aligned(16))) float Zs[256 * 16];   // dZ tile [voxel][co], zero outside the plane
  __shared__ float red[4][2][256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, g = lane >> 4;
  // Both MFMA operands come straight from LDS reads (as in every other kernel here).  Taps >= NT (rows of D nobody
  // reads) simply alias tap 0.  NB: a first version masked them with a VALU multiply and zero-initialised dZ in a
  // register before a predicated load; hipcc (ROCm 7.2, gfx950) then scheduled VALU writes of the operand registers
  // right around the MFMA and the single-accumulator (DEPTH = 1) chain produced wrong rows on the hardware.
  const int t0 = li < NT ? li : 0, t1 = li + 16 < NT ? li + 16 : 0;
  const int off0 = (t0 / 9) * NP + ((t0 % 9) / 3) * HW_ + t0 % 3;
  const int off1 = (t1 / 9) * NP + ((t1 % 9) / 3) * HW_ + t1 % 3;
  const int tiles_x = (a.W + TW - 1) / TW, tiles_y = (a.H + TH - 1) / TH;
  const long n_tiles = (long)a.NB * tiles_y * tiles_x;
  f32x4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
  for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int tx = t % tiles_x; const long r = t / tiles_x; const int ty = r % tiles_y; const int pl = r / tiles_y;
    const int xd = pl % a.D3;
    __syncthreads();
    for (int u = tid; u < DEPTH * NP; u += 256) {
      const int k = u / NP, hp = u - k * NP, hy = hp / HW_, hx = hp - hy * HW_;
      const int gy = ty * TH + hy - 1, gx = tx * TW + hx - 1, dk = k - DEPTH / 2, pz = xd + dk;
      Xs[u] = (pz >= 0 && pz < a.D3 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
                  ? a.Ain[(((long)(pl + dk) * a.H + gy) * a.W + gx) * a.lda] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = tid + 256 * i, p = u >> 2, q = u & 3;
      const int gy = ty * TH + (p >> 4), gx = tx * TW + (p & 15);
      f32x4 v = {0, 0, 0, 0};
      if (gy < a.H && gx < a.W && 4 * q < a.Cout) {
        const long zo = (((long)pl * a.H + gy) * a.W + gx) * a.ldz + 4 * q;
        if (a.mma == 4) v = __builtin_convertvector(*reinterpret_cast<const f16x4*>(reinterpret_cast<const _Float16*>(a.dZ) + zo), f32x4);
        else v = *reinterpret_cast<const f32x4*>(a.dZ + zo);
      }
      *reinterpret_cast<f32x4*>(&Zs[p * 16 + 4 * q]) = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {                               // wave w: voxels 64w .. 64w+63 of the tile, 4 per step
      const int p = 64 * w + 4 * s + g;
      const float z = Zs[p * 16 + li];
      const float* xb = Xs + (p >> 4) * HW_ + (p & 15);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[off0], z, acc0, 0, 0, 0);
      if (DEPTH == 3) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[off1], z, acc1, 0, 0, 0);
    }
  }
  // lane holds D[tap = 16*h + 4g + r][co = li]; sum the four waves, then one slab per workgroup
#pragma unroll
  for (int r = 0; r < 4; ++r) { red[w][0][(4 * g + r) * 16 + li] = acc0[r]; red[w][1][(4 * g + r) * 16 + li] = acc1[r]; }
  __syncthreads();
  for (int u = tid; u < 512; u += 256) {
    const int h = u >> 8, e = u & 255, tap = 16 * h + (e >> 4), co = e & 15;
    if (tap < NT) {
      const float v = (red[0][h][e] + red[1][h][e]) + (red[2][h][e] + red[3][h][e]);
      a.partial[(((long)blockIdx.x * a.taps + tap) * a.CoutPad + co) * a.CinPad] = v;
    }
  }
}

// EL consecutive slab elements x GR slab groups per 512-thread block.  <16, 32> for launches with many slabs (a
// 9 x 32 x 32 block has only 144 workgroups at 64 elements each, streaming 19 MB: latency-bound at 11 us); <64, 8>
// when there are few slabs (most of 32 groups would idle).  Slab layout [tap][co][ci], dW torch layout.
template <int EL, int GR>
__global__ __launch_bounds__(512) void wgrad_reduce_kernel(const float* __restrict__ partial, int chunks, int taps, int CoutPad, int CinPad,
                                    int Cout, int Cin, float* __restrict__ dW, int accumulate) {
  __shared__ float red[GR][EL];
  const int tx = threadIdx.x % EL, ty = threadIdx.x / EL;
  const long j = (long)blockIdx.x * EL + tx;
  const long tot = (long)taps * Cout * Cin;
  float s0 = 0.f, s1 = 0.f;
  int ci = 0, co = 0, tap = 0;
  if (j < tot) {
    ci = j % Cin; const long r = j / Cin; co = r % Cout; tap = r / Cout;
    const long off = ((long)tap * CoutPad + co) * CinPad + ci, stride = (long)taps * CoutPad * CinPad;
    int c = ty;
    for (; c + GR < chunks; c += 2 * GR) { s0 += partial[off + (long)c * stride]; s1 += partial[off + (long)(c + GR) * stride]; }
    for (; c < chunks; c += GR) s0 += partial[off + (long)c * stride];
  }
  red[ty][tx] = s0 + s1;
  __syncthreads();
  if (ty == 0 && j < tot) {
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < GR; g += 4) s += (red[g][tx] + red[g + 1][tx]) + (red[g + 2][tx] + red[g + 3][tx]);
    const long o = ((long)co * Cin + ci) * taps + tap;
    dW[o] = accumulate ? dW[o] + s : s;
  }
}
// <16,32> with four consecutive elements (one 16-byte load per slab) per thread: 256-byte runs per slab instead of 64-byte
// ones, a quarter of the blocks.  Same per-element summation order as wgrad_reduce_kernel<16,32> (bit-identical).
__global__ __launch_bounds__(512) void wgrad_reduce4_kernel(const float* __restrict__ partial, int chunks, int taps, int CoutPad, int CinPad,
                                                           int Cout, int Cin, float* __restrict__ dW, int accumulate) {
  constexpr int EL4 = 16, GR = 32;
  __shared__ f32x4 red[GR][EL4];
  const int tx = threadIdx.x % EL4, ty = threadIdx.x / EL4;
  const long j = ((long)blockIdx.x * EL4 + tx) * 4;
  const long tot = (long)taps * Cout * Cin;
  f32x4 s0 = {0, 0, 0, 0}, s1 = {0, 0, 0, 0};
  int ci = 0, co = 0, tap = 0;
  if (j < tot) {
    ci = j % Cin; const long r = j / Cin; co = r % Cout; tap = r / Cout;
    const long off = ((long)tap * CoutPad + co) * CinPad + ci, stride = (long)taps * CoutPad * CinPad;
    int c = ty;
    for (; c + GR < chunks; c += 2 * GR) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(partial + off + (long)c * stride);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(partial + off + (long)(c + GR) * stride);
      s0 += v0; s1 += v1;
    }
    for (; c < chunks; c += GR) s0 += *reinterpret_cast<const f32x4*>(partial + off + (long)c * stride);
  }
  red[ty][tx] = s0 + s1;
  __syncthreads();
  if (ty == 0 && j < tot) {
    f32x4 sv = {0, 0, 0, 0};
#pragma unroll
    for (int g = 0; g < GR; g += 4) sv += (red[g][tx] + red[g + 1][tx]) + (red[g + 2][tx] + red[g + 3][tx]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long o = ((long)co * Cin + ci + e) * taps + tap;
      dW[o] = accumulate ? dW[o] + sv[e] : sv[e];
    }
  }
}
// which slab reduction follows a launch of `chunks` slabs: 1 wgrad_reduce_kernel<64,8>, 2 wgrad_reduce_kernel<16,32>, 3 wgrad_reduce4_kernel
int wgrad_reduce_kind(long chunks, int taps, int CinPad, int Cout, int Cin) {
  const long tot = (long)Cout * Cin * taps;
  if (chunks > 16 && (Cin & 3) == 0 && (CinPad & 3) == 0 && tot >= 64 * 64) return 3;
  return chunks > 16 ? 2 : 1;
}
void launch_wgrad_reduce(hipStream_t st, const float* ws, int chunks, int taps, int CoutPad, int CinPad, int Cout, int Cin,
                                float* dW, int accumulate) {
  const long tot = (long)Cout * Cin * taps;
  const int kind = wgrad_reduce_kind(chunks, taps, CinPad, Cout, Cin);
  if (kind == 3)
    hipLaunchKernelGGL(wgrad_reduce4_kernel, dim3((unsigned)((tot / 4 + 15) / 16)), dim3(512), 0, st, ws, chunks, taps, CoutPad, CinPad, Cout, Cin, dW, accumulate);
  else if (kind == 2)
    hipLaunchKernelGGL((wgrad_reduce_kernel<16, 32>), dim3((tot + 15) / 16), dim3(512), 0, st, ws, chunks, taps, CoutPad, CinPad, Cout, Cin, dW, accumulate);
  else
    hipLaunchKernelGGL((wgrad_reduce_kernel<64, 8>), dim3((tot + 63) / 64), dim3(512), 0, st, ws, chunks, taps, CoutPad, CinPad, Cout, Cin, dW, accumulate);
}

// column sums (bias gradient): out[c] = sum_pix X[pix][c].  float4 lanes along channels,
// rows strided over the block, per-block slabs + fp64 fixed-order finalize.
template <typename T>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const T* __restrict__ X, long ldx, long M, int C,
                                                            float* __restrict__ partial) {
  const long rpb = (M + gridDim.x - 1) / gridDim.x;
  const long r0 = blockIdx.x * rpb, r1 = min(M, r0 + rpb);
  extern __shared__ __attribute__((aligned(16))) float red[];   // [256][4]
  if ((C & 3) == 0 && (ldx & 3) == 0 && C <= 1024) {
    const int q4 = C / 4, tq = threadIdx.x % q4, tr = threadIdx.x / q4, rstep = 256 / q4;
    f32x4 s = {0, 0, 0, 0};
    if (tr < rstep)
      for (long r = r0 + tr; r < r1; r += rstep) s += ld4f(X + r * ldx + 4 * tq);
    *reinterpret_cast<f32x4*>(&red[threadIdx.x * 4]) = s;
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
      const int qq = c / 4, e = c % 4;
      float a = 0.f;
      for (int r = 0; r < rstep; ++r) a += red[(r * q4 + qq) * 4 + e];
      partial[(long)blockIdx.x * C + c] = a;
    }
  } else if (C <= 256) {
    // narrow / odd channel counts (the 2-class out_conv of the V-Net: 4 M rows x 2 channels): thread = (row lane, channel)
    const int rstep = 256 / C, c = threadIdx.x % C, tr = threadIdx.x / C;
    float s = 0.f;
    if (tr < rstep)
      for (long r = r0 + tr; r < r1; r += rstep) s += (float)X[r * ldx + c];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < C) {
      float a = 0.f;
      for (int r = 0; r < rstep; ++r) a += red[r * C + threadIdx.x];
      partial[(long)blockIdx.x * C + threadIdx.x] = a;
    }
  } else {
    for (int c = threadIdx.x; c < C; c += 256) {
      float s = 0.f;
      for (long r = r0; r < r1; ++r) s += (float)X[r * ldx + c];
      partial[(long)blockIdx.x * C + c] = s;
    }
  }
}
__global__ __launch_bounds__(64) void colsum_final_kernel(const float* __restrict__ partial, int nblk, int C, float* __restrict__ out, int accumulate) {
  const int c = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 64) s += (double)partial[(long)b * C + c];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) out[c] = accumulate ? out[c] + (float)s : (float)s;
}

// ---- the weight-gradient route: kernel, tile, flat or rectangular, slab count and reduction, in pure host code ------------------------
constexpr long WGRAD_TARGET_BLOCKS = 512;      // two resident workgroups per CU, several tiles each
// the channel tiles: 16 / 32 / 64 for the GEMM-form kernels (1x1, and the f16 1x1x1), 16 / 32 for the spatial ones (3x3, 3x3x3)
static int wg_tile1(int c) { return c >= 64 ? 64 : (c > 16 ? 32 : 16); }
static int wg_tile9(int c) { return c > 16 ? 32 : 16; }
static int pad_to(int c, int t) { return (c + t - 1) / t * t; }

// floats of workspace that any route of this shape may ask for: the reservation wgrad_plan_finish clamps its slab count to
extern "C" long arco_wgrad_ws_floats(int Cout, int Cin, int taps, long M) {
  const long n_tiles = (M + 127) / 128 * 4 + 64;   // upper bound incl. ragged spatial tiles
  if (taps >= 9) {
    const int hco = wg_tile9(Cout), hci = wg_tile9(Cin);
    const long cop = pad_to(Cout, hco), cip = pad_to(Cin, hci);
    long chunks = 1536 / ((taps / 9) * (cop / hco) * (cip / hci)); if (chunks > n_tiles) chunks = n_tiles; if (chunks < 1) chunks = 1;
    return chunks * taps * cop * cip;
  }
  const int co_b = wg_tile1(Cout), ci_b = wg_tile1(Cin);
  const int CoutPad = pad_to(Cout, co_b), CinPad = pad_to(Cin, ci_b);
  const long yz = (long)(CoutPad / co_b) * (CinPad / ci_b) * taps;
  long chunks = 2048 / yz; if (chunks < 1) chunks = 1; if (chunks > n_tiles) chunks = n_tiles;
  return chunks * taps * CoutPad * CinPad;
}
static int wgrad_plan_finish(WgradPlan& p, int tapform, int fam, int var, int cob, int cib, long slabs, int taps, int Cout, int Cin, long M) {
  p.family = fam; p.cob = cob; p.cib = cib;
  p.slab_floats = (long)taps * p.CoutPad * p.CinPad;
  // one slab per workgroup, and never more slabs than arco_wgrad_ws_floats reserves for the same (Cout, Cin, taps, M): its bound
  // ceil(M / 128) * 4 + 64 is below the tile count of a batch of many small planes (200 maps of 4 x 4: 200 tiles, 164 slabs).  Every
  // kernel strides its tiles by gridDim.x, so fewer workgroups compute the same sums.
  const long reserved = arco_wgrad_ws_floats(Cout, Cin, taps, M) / p.slab_floats;
  if (slabs < 1) slabs = 1;
  if (slabs > reserved) slabs = reserved;
  if (slabs < 1) return ARCO_ERR_UNSUPPORTED;
  p.slabs = slabs;
  p.reduce = wgrad_reduce_kind(slabs, taps, p.CinPad, Cout, Cin);
  p.route = tapform * 1000000 + fam * 100000 + var * 10000 + cob * 100 + cib;
  return ARCO_OK;
}

int wgrad_plan(int entry, int taps, int NV, int D3, int H, int W, int Cin, int Cout, long ld_dz, long ld_in, int mma, bool pro_on,
               int pro_groups, bool aligned16, WgradPlan& p) {
  p = WgradPlan{};
  const int NB = NV * D3;
  const long M = (long)NB * H * W;
  p.ydim = p.zdim = 1;
  if (entry == 1) {      // arco_conv3x3_image_wgrad_h: f16 dZ of 16 channels against the fp32 image of Cin <= 4 channels
    if (taps != 9 || Cout != 16 || (ld_dz & 7) != 0 || !aligned16) return ARCO_ERR_UNSUPPORTED;
    p.CoutPad = 16; p.CinPad = 16;
    const long tiles = (long)NB * ((H + 15) / 16) * ((W + 15) / 16);
    p.n_tiles = (int)tiles;
    return wgrad_plan_finish(p, 9, WG_F_HIMAGE, 0, 16, Cin, tiles < 512 ? tiles : 512, taps, Cout, Cin, M);
  }
  if (pro_on) {          // arco_conv3d_wgrad_pro: (the 3x3x3 consumer-side activation exists in the forward kernel only: gradient-free passes)
    if (taps != 9) return ARCO_ERR_UNSUPPORTED;
    if (!arco_conv_pro_ok(taps, NV, D3, H, W, Cin, Cout, ld_in, mma, pro_groups) || (ld_dz & 3) != 0) return ARCO_ERR_UNSUPPORTED;
  }
  if (mma == 4 && !(taps >= 9 && Cin == 1)) {     // f16 activation storage (dZ and in are f16; the first layer's input volume is fp32): conv_h.hip
    // (2-D 3x3: dZ rows of any width are staged element-wise when they are not whole 16-byte pieces - the U-Net's 19-class out_conv)
    if ((Cin & 7) != 0 || (ld_in & 7) != 0 || ((ld_dz & 1) != 0 && taps != 9)) return ARCO_ERR_UNSUPPORTED;
    if (taps >= 9) {
      const int hco = wg_tile9(Cout), hci = wg_tile9(Cin);
      p.CoutPad = pad_to(Cout, hco); p.CinPad = pad_to(Cin, hci);
      p.n_tiles = NB * ((H + 7) / 8) * ((W + 15) / 16);
      p.zdim = taps / 9; p.ydim = (p.CoutPad / hco) * (p.CinPad / hci);
      long chunks = WGRAD_TARGET_BLOCKS / ((long)p.zdim * p.ydim); if (chunks > p.n_tiles) chunks = p.n_tiles;
      return wgrad_plan_finish(p, 9, WG_F_HGRAD, 0, hco, hci, chunks, taps, Cout, Cin, M);
    }
    const int co_b = wg_tile1(Cout), ci_b = wg_tile1(Cin);
    p.CoutPad = pad_to(Cout, co_b); p.CinPad = pad_to(Cin, ci_b);
    p.n_tiles = (int)((M + 127) / 128);
    p.ydim = (p.CoutPad / co_b) * (p.CinPad / ci_b);
    long chunks = WGRAD_TARGET_BLOCKS / p.ydim; if (chunks < 1) chunks = 1; if (chunks > p.n_tiles) chunks = p.n_tiles;
    return wgrad_plan_finish(p, 1, WG_F_HGRAD, 0, co_b, ci_b, chunks, taps, Cout, Cin, M);
  }
  const int amma = mma >= 3 ? mma : ((taps == 27 && mma) ? 2 : 0);   // 1 / 2: bf16 operands (gradients: range); 3: split-bf16 (fp32-accurate)
  const int co_b = wg_tile1(Cout), ci_b = wg_tile1(Cin);
  p.CoutPad = pad_to(Cout, co_b); p.CinPad = pad_to(Cin, ci_b);
  p.n_tiles = taps >= 9 ? NB * ((H + 7) / 8) * ((W + 15) / 16) : (int)((M + 127) / 128);
  if (taps >= 9 && Cin == 1 && Cout <= 16 && (Cout & 3) == 0 && (ld_dz & 3) == 0) {   // one-channel input (first layer of both nets): taps as M
    if (pro_on) return ARCO_ERR_UNSUPPORTED;
    p.CoutPad = 16; p.CinPad = 16;
    const long tiles = (long)NB * ((H + 15) / 16) * ((W + 15) / 16);
    p.n_tiles = (int)tiles;
    return wgrad_plan_finish(p, 9, WG_F_IMAGE, taps / 9, 16, 16, tiles < 512 ? tiles : 512, taps, Cout, Cin, M);
  }
  // f16 dZ against the one-channel fp32 volume exists in wgrad_image3d_kernel only: the kernels below would read the f16 rows as fp32
  if (amma == 4) return ARCO_ERR_UNSUPPORTED;
  if (taps >= 9) {       // spatial kernels: all taps of a plane per block, operands staged once (halo in LDS)
    const int hco = wg_tile9(Cout), hci = wg_tile9(Cin);
    p.CoutPad = pad_to(Cout, hco); p.CinPad = pad_to(Cin, hci);
    // narrow planes (W not a multiple of 16): flat-position tiles for the fp32 / reduced-precision kernels.  In split-bf16 mode
    // the rectangular 8 x 16 tiles of wgrad_split_kernel are taken instead, ragged last column of tiles and all (W = 40: 17 %
    // of the MFMA rows idle, W = 20 / 10: 37 %) - six bf16 MFMAs per 32 pixels still beat eight fp32 MFMAs per 16 by more than
    // that (the fp32 flat-tile kernel was the earlier choice there)
    const bool split_ok = amma == 3 && (Cout & 3) == 0 && (Cin & 3) == 0 && (ld_dz & 3) == 0 && (ld_in & 3) == 0;
    p.flat = (W & 15) != 0 && W + 2 <= IGEMM_FLAT_WPMAX && !(split_ok && W >= 10);
    if (p.flat) p.n_tiles = NB * ((H * (W + 2) + 127) / 128);
    p.zdim = taps / 9; p.ydim = (p.CoutPad / hco) * (p.CinPad / hci);
    // 32x32 blocks run persistent (2 workgroups per CU, several tiles each); the others one slab per ~tile
    // (16 x 32 blocks of the split kernel: 60.7 KB of LDS, two per CU as well - 768 left a third round at half occupancy)
    const long target = (hci == 32 && (hco == 32 || amma == 3)) ? WGRAD_TARGET_BLOCKS : 768;
    long chunks = target / ((long)p.zdim * p.ydim); if (chunks > p.n_tiles) chunks = p.n_tiles;
    const bool split = split_ok && !p.flat;
    if (pro_on && !split) return ARCO_ERR_UNSUPPORTED;
    if (split) return wgrad_plan_finish(p, 9, WG_F_SPLIT, pro_on ? 1 : 0, hco, hci, chunks, taps, Cout, Cin, M);
    p.bf16 = amma == 2;
    return wgrad_plan_finish(p, 9, WG_F_HALO, (p.flat ? 1 : 0) + (p.bf16 ? 2 : 0), hco, hci, chunks, taps, Cout, Cin, M);
  }
  {   // wide 1x1 gradients over many pixels: 128 x 128 blocks of 64-pixel tiles, two workgroups per CU (wgrad_q_kernel)
    const int cop = pad_to(Cout, 128), cip = pad_to(Cin, 128);
    const long yzq = (long)(cop / 128) * (cip / 128);
    const long reserved = arco_wgrad_ws_floats(Cout, Cin, taps, M);
    long chq = 256 / yzq; if (chq < 1) chq = 1; if (chq > p.n_tiles) chq = p.n_tiles;
    if (taps == 1 && Cout >= 192 && Cin >= 192 && M >= 32768 && (Cout & 3) == 0 && (Cin & 3) == 0 &&
        (ld_dz & 3) == 0 && (ld_in & 3) == 0 && aligned16 && chq * cop * cip <= reserved) {
      p.CoutPad = cop; p.CinPad = cip;
      p.ydim = cop / 128; p.zdim = cip / 128;
      p.n_tiles = (int)((M + 63) / 64);
      long ch2 = WGRAD_TARGET_BLOCKS / yzq; if (ch2 < 1) ch2 = 1; if (ch2 > p.n_tiles) ch2 = p.n_tiles;
      if (ch2 * cop * cip <= reserved) chq = ch2;
      return wgrad_plan_finish(p, 1, WG_F_Q, 0, 0, 64, chq, taps, Cout, Cin, M);
    }
  }
  p.ydim = p.CoutPad / co_b; p.zdim = (p.CinPad / ci_b) * taps;
  const long yz = (long)p.ydim * p.zdim;
  // two resident workgroups per CU, 6-13 tiles each (2048: 3 tiles each, a third of them behind an exposed first fetch; 4x the slabs)
  long chunks = WGRAD_TARGET_BLOCKS / yz; if (chunks < 1) chunks = 1; if (chunks > p.n_tiles) chunks = p.n_tiles;
  return wgrad_plan_finish(p, 1, WG_F_GEMM, 0, co_b, ci_b, chunks, taps, Cout, Cin, M);
}

// ---- launch: one typed launcher per tiled kernel family, and the switch from the plan's (cob, cib) to the instantiation -------------
constexpr size_t WG_RED9_BYTES = (size_t)4 * 9 * 256 * 4;      // the cross-wave sum of the 3x3 kernels whose four waves share sub-tiles
template <int COB, int CIB>
static void launch_wgrad_gemm(dim3 grid, hipStream_t st, const WgradArgs& a) {
  constexpr int LZ = (COB % 32 == 0) ? COB + WGRAD1_PAD : COB, LA = (CIB % 32 == 0) ? CIB + WGRAD1_PAD : CIB;
  size_t sh = (size_t)128 * (LZ + LA) * 4; const size_t rd = (size_t)4 * COB * CIB * 4;
  if (sh < rd) sh = rd;
  arco_launch<wgrad_kernel<COB, CIB>>(grid, dim3(256), sh, sh > 64 * 1024 ? sh : 0, st, a);
}
template <int COB, int CIB>
static void launch_wgrad_halo(bool flat, dim3 grid, hipStream_t st, const WgradArgs& a) {
  constexpr int LZ = (COB % 32 == 0) ? COB + 16 : COB, LA = (CIB % 32 == 0) ? CIB + 16 : CIB;
  size_t sh = (size_t)(128 * LZ + (flat ? 128 + 2 * (a.W + 2) + 2 : 180) * LA) * 4;
  if (sh < WG_RED9_BYTES && (COB / 16) * (CIB / 16) < 4) sh = WG_RED9_BYTES;
  // flat tiles: the limit is raised to the widest plane's figure whatever this W, so that one raise serves every later launch
  constexpr size_t flat_max = (size_t)(128 * LZ + (128 + 2 * IGEMM_FLAT_WPMAX + 2) * LA) * 4;
  if (flat && a.mma == 2) arco_launch<wgrad_halo2_kernel<COB, CIB, true, 2>>(grid, dim3(256), sh, flat_max, st, a);
  else if (flat) arco_launch<wgrad_halo2_kernel<COB, CIB, true>>(grid, dim3(256), sh, flat_max, st, a);
  else if (a.mma == 2) arco_launch<wgrad_halo2_kernel<COB, CIB, false, 2>>(grid, dim3(256), sh, 0, st, a);
  else arco_launch<wgrad_halo2_kernel<COB, CIB>>(grid, dim3(256), sh, 0, st, a);
}
template <int COB, int CIB>
static void launch_wgrad_split(dim3 grid, hipStream_t st, const WgradArgs& a) {
  size_t sh = (size_t)(3 * COB * WG_CSZ + 3 * CIB * WG_CSX) * 4;
  if (sh < WG_RED9_BYTES && (COB / 16) * (CIB / 16) < 4) sh = WG_RED9_BYTES;
  const size_t raise = sh > 64 * 1024 ? sh : 0;
  if (a.pro.mean) arco_launch<wgrad_split_kernel<COB, CIB, true>>(grid, dim3(256), sh, raise, st, a);
  else arco_launch<wgrad_split_kernel<COB, CIB>>(grid, dim3(256), sh, raise, st, a);
}
template <int COB, int CIB>
static void launch_wgrad_tile(const WgradPlan& p, dim3 grid, hipStream_t st, const WgradArgs& a) {
  if constexpr (COB <= 32 && CIB <= 32) {      // the spatial kernels exist with 16 / 32 channel tiles only (wg_tile9)
    if (p.family == WG_F_SPLIT) return launch_wgrad_split<COB, CIB>(grid, st, a);
    if (p.family == WG_F_HALO) return launch_wgrad_halo<COB, CIB>(p.flat, grid, st, a);
  }
  launch_wgrad_gemm<COB, CIB>(grid, st, a);
}
template <int COB>
static void launch_wgrad_cib(const WgradPlan& p, dim3 grid, hipStream_t st, const WgradArgs& a) {
  if (p.cib == 64) launch_wgrad_tile<COB, 64>(p, grid, st, a);
  else if (p.cib == 32) launch_wgrad_tile<COB, 32>(p, grid, st, a);
  else launch_wgrad_tile<COB, 16>(p, grid, st, a);
}
static void launch_wgrad_tiled(const WgradPlan& p, dim3 grid, hipStream_t st, const WgradArgs& a) {
  if (p.cob == 64) launch_wgrad_cib<64>(p, grid, st, a);
  else if (p.cob == 32) launch_wgrad_cib<32>(p, grid, st, a);
  else launch_wgrad_cib<16>(p, grid, st, a);
}

static int conv3d_wgrad_impl(const float* dZ, long ld_dz, int Cout, const float* in, long ld_in, int Cin, int taps, int NV,
                             int D3, int H, int W, float* ws, float* dW, int accumulate, int mma, const ArcoActPro* pro, void* stream) {
  ARCO_CHECK_ARG(dZ && in && ws && dW && (taps == 1 || taps == 9 || taps == 27) && mma >= 0 && mma <= 4 && Cout > 0 && Cin > 0 && NV > 0 &&
                 D3 > 0 && H > 0 && W > 0 && ld_dz >= Cout && ld_in >= Cin && (accumulate == 0 || accumulate == 1));
  const int NB = NV * D3;
  arco_note_wgrad_route(0);
  WgradPlan p;
  const bool aligned16 = (reinterpret_cast<uintptr_t>(dZ) & 15) == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;
  const int rc = wgrad_plan(0, taps, NV, D3, H, W, Cin, Cout, ld_dz, ld_in, mma, pro != nullptr, pro ? pro->groups : 0, aligned16, p);
  if (rc != ARCO_OK) return rc;
  hipStream_t st = as_stream(stream);
  if (p.family == WG_F_HGRAD) {
    const int r = hwgrad_dispatch(dZ, ld_dz, Cout, in, ld_in, Cin, taps, NB, D3, H, W, ws, p, as_stream(stream));
    if (r != ARCO_OK) return r;
    arco_note_wgrad_route(p.route);
    launch_wgrad_reduce(st, ws, (int)p.slabs, taps, p.CoutPad, p.CinPad, Cout, Cin, dW, accumulate);
    return arco_launch_status();
  }
  WgradArgs a{};
  a.D3 = D3; a.mma = mma >= 3 ? mma : ((taps == 27 && mma) ? 2 : 0);
  a.dZ = dZ; a.ldz = ld_dz; a.Cout = Cout; a.Ain = in; a.lda = ld_in; a.Cin = Cin; a.taps = taps;
  a.NB = NB; a.H = H; a.W = W; a.M = (long)NB * H * W; a.partial = ws;
  static const int abl = getenv("ARCO_WGRAD_ABL") ? atoi(getenv("ARCO_WGRAD_ABL")) : 0;
  a.abl = abl;
  if (pro) a.pro = *pro;
  a.CoutPad = p.CoutPad; a.CinPad = p.CinPad; a.n_tiles = p.n_tiles;
  const long chunks = p.slabs;
  const dim3 grid((unsigned)chunks, p.ydim, p.zdim);
  if (p.family == WG_F_IMAGE) {
    if (taps == 9) a.D3 = 1;
    if (taps == 27) arco_launch<wgrad_image3d_kernel<3>>(grid, dim3(256), 0, 0, st, a);
    else arco_launch<wgrad_image3d_kernel<1>>(grid, dim3(256), 0, 0, st, a);
  } else if (p.family == WG_F_Q) {
    constexpr int shq = 64 * (2 * (128 + WGRAD1_PAD)) * 4;
    arco_launch<wgrad_q_kernel<64>>(grid, dim3(256), shq, shq, st, a);
  } else {
    launch_wgrad_tiled(p, grid, st, a);
  }
  arco_note_wgrad_route(p.route);
  launch_wgrad_reduce(st, ws, (int)chunks, taps, a.CoutPad, a.CinPad, Cout, Cin, dW, accumulate);
  return arco_launch_status();
}

// The first 2-D layer under f16 activation storage: dW[co][ci][tap] = sum_pix dZ[pix][co] X[pix + tap][ci] from the f16 dZ (16
// channels) and the fp32 IMAGE (1 - 4 channels).  A thread owns one (co, tap, ci) element (up to 576 of them) over a 16 x 16 tile
// staged in LDS, one slab per persistent workgroup -> wgrad_reduce (fixed order, deterministic).
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
      if (gy < H && gx < W) v = ldv<_Float16, 8>(dZ + (((long)nb * H + gy) * W + gx) * ldz + 8 * q);
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

template <typename T>
static int colsum_impl(const T* X, long ldx, long M, int C, float* ws, float* out, int accumulate, void* stream) {
  ARCO_CHECK_ARG(X && ws && out && M > 0 && C > 0 && ldx >= C && (accumulate == 0 || accumulate == 1));
  int nblk = (int)((M + 511) / 512); if (nblk > 1024) nblk = 1024; if (nblk < 1) nblk = 1;
  hipLaunchKernelGGL(colsum_partial_kernel<T>, dim3(nblk), dim3(256), 1024 * sizeof(float), as_stream(stream), X, ldx, M, C, ws);
  hipLaunchKernelGGL(colsum_final_kernel, dim3(C), dim3(64), 0, as_stream(stream), ws, nblk, C, out, accumulate);
  return arco_launch_status();
}

thread_local int arco_wgrad_route = 0;

extern "C" {

// Test-facing: the id of the kernel that the most recent weight-gradient launch of this thread took (arco_conv_wgrad, arco_conv3d_wgrad(_pro),
// arco_conv3x3_image_wgrad_h, the f16 kernels of conv_h.hip included); 0 before the first launch and after a call that found no kernel
// (ARCO_ERR_UNSUPPORTED); a call rejected with ARCO_ERR_ARG leaves it unchanged.  Host side only: one thread-local store per launch.
int arco_wgrad_last_route(void) { return arco_wgrad_route; }

// Query: the route wgrad_plan chooses - the function the launch itself calls.  Returns the kernel id or ARCO_ERR_UNSUPPORTED;
// *slabs = workgroups along x = slabs written to ws, *slab_floats = floats per slab, *reduce = 1 wgrad_reduce_kernel<64,8>,
// 2 wgrad_reduce_kernel<16,32>, 3 wgrad_reduce4_kernel (each may be NULL).
int arco_wgrad_config(int entry, int taps, int NV, int D3, int H, int W, int Cin, int Cout, long ld_dz, long ld_in, int mma,
                      int pro_groups, int aligned16, long* slabs, long* slab_floats, int* reduce) {
  ARCO_CHECK_ARG((entry == 0 || entry == 1) && (taps == 1 || taps == 9 || taps == 27) && mma >= 0 && mma <= 4 && NV > 0 && D3 > 0 && H > 0 &&
                 W > 0 && Cin > 0 && Cout > 0 && ld_dz >= Cout && ld_in >= Cin && pro_groups >= 0 &&
                 (entry == 0 || (Cin <= 4 && D3 == 1 && taps == 9)));
  WgradPlan p;
  const int rc = wgrad_plan(entry, taps, NV, D3, H, W, Cin, Cout, ld_dz, ld_in, mma, pro_groups > 0, pro_groups, aligned16 != 0, p);
  if (rc != ARCO_OK) return rc;
  if (slabs) *slabs = p.slabs;
  if (slab_floats) *slab_floats = p.slab_floats;
  if (reduce) *reduce = p.reduce;
  return p.route;
}

int arco_conv3d_wgrad(const float* dZ, long ld_dz, int Cout, const float* in, long ld_in, int Cin, int taps, int NV,
                      int D3, int H, int W, float* ws, float* dW, int accumulate, int mma, void* stream) {
  return conv3d_wgrad_impl(dZ, ld_dz, Cout, in, ld_in, Cin, taps, NV, D3, H, W, ws, dW, accumulate, mma, nullptr, stream);
}
// ... where `in` is the pre-activation z of the producing convolution (see arco_conv3d_fwd_pro): dW = dZ^T . act(z)
int arco_conv3d_wgrad_pro(const float* dZ, long ld_dz, int Cout, const float* in, long ld_in, int Cin, int taps, int NV,
                          int D3, int H, int W, float* ws, float* dW, int accumulate, int mma, const ArcoActPro* pro, void* stream) {
  ARCO_CHECK_ARG(pro && pro->mean && pro->istd && pro->gamma && pro->beta && pro->groups >= 1 && (pro->drop_mode == 0 || pro->drop_mode == 1) &&
                 pro->p >= 0.f && pro->p < 1.f);
  return conv3d_wgrad_impl(dZ, ld_dz, Cout, in, ld_in, Cin, taps, NV, D3, H, W, ws, dW, accumulate, mma, pro, stream);
}

int arco_conv_wgrad(const float* dZ, long ld_dz, int Cout, const float* in, long ld_in, int Cin, int taps, int NB,
                    int H, int W, float* ws, float* dW, int accumulate, void* stream) {
  return arco_conv3d_wgrad(dZ, ld_dz, Cout, in, ld_in, Cin, taps, NB, 1, H, W, ws, dW, accumulate, 0, stream);
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

// out[c] (+)= sum over pixels of X[pix][c];  ws holds 1024*C floats
int arco_colsum(const float* X, long ldx, long M, int C, float* ws, float* out, int accumulate, void* stream) {
  return colsum_impl(X, ldx, M, C, ws, out, accumulate, stream);
}
// the same over an f16 tensor (f16 activation storage: bias gradients of the V-Net's convolutions)
int arco_colsum_h(const void* X, long ldx, long M, int C, float* ws, float* out, int accumulate, void* stream) {
  return colsum_impl(reinterpret_cast<const _Float16*>(X), ldx, M, C, ws, out, accumulate, stream);
}

}  // extern "C"
