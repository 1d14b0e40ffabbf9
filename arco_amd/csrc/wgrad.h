// The weight-gradient family shared by wgrad.hip (fp32 / bf16 / split-bf16 kernels) and conv_h.hip (f16 activation storage).
#pragma once
#include "igemm_args.h"

// wgrad.hip: the weight-gradient route of a shape, decided in pure host code.  conv3d_wgrad_impl, hwgrad_dispatch and
// arco_conv3x3_image_wgrad_h launch what wgrad_plan returns and the query arco_wgrad_config reports the same record, so the launch
// and the query cannot drift apart.  Ids (include/arco_hip.h): T*1e6 + F*1e5 + V*1e4 + COB*100 + CIB.
enum { WG_F_GEMM = 0, WG_F_Q = 1, WG_F_HALO = 2, WG_F_SPLIT = 3, WG_F_IMAGE = 4, WG_F_HGRAD = 5, WG_F_HIMAGE = 6 };
struct WgradPlan {
  int route;                  // kernel id, 0 when no kernel takes the shape
  int family, cob, cib;       // WG_F_*, the channel tile (wgrad_q_kernel: cob = 0, cib = pixels per step)
  bool flat, bf16;            // wgrad_halo2_kernel: flat-position tiles, bf16 operands
  int CoutPad, CinPad, n_tiles, ydim, zdim;
  long slabs, slab_floats;    // grid.x = slabs, one slab [taps][CoutPad][CinPad] per workgroup: slabs * slab_floats <= arco_wgrad_ws_floats
  int reduce;                 // 1 wgrad_reduce_kernel<64,8>, 2 wgrad_reduce_kernel<16,32>, 3 wgrad_reduce4_kernel
};
// entry 0: arco_conv3d_wgrad(_pro) (pro_on: with a consumer-side activation of pro_groups BatchNorm groups); 1: arco_conv3x3_image_wgrad_h.  aligned16: dZ and `in`
// start on 16-byte boundaries.  Returns ARCO_OK or ARCO_ERR_UNSUPPORTED (p.route = 0).
int wgrad_plan(int entry, int taps, int NV, int D3, int H, int W, int Cin, int Cout, long ld_dz, long ld_in, int mma, bool pro_on,
               int pro_groups, bool aligned16, WgradPlan& p);
int wgrad_reduce_kind(long chunks, int taps, int CinPad, int Cout, int Cin);
extern thread_local int arco_wgrad_route;
static inline void arco_note_wgrad_route(int id) { arco_wgrad_route = id; }
// conv_h.hip: the slabs of the weight gradient from f16 dZ / X (fp32, in ws), launched as wgrad_plan laid it out; the caller reduces
int hwgrad_dispatch(const void* dZ, long ld_dz, int Cout, const void* in, long ld_in, int Cin, int taps, int NB, int D3, int H, int W,
                    float* ws, const WgradPlan& p, hipStream_t st);
// wgrad.hip: fixed-order sum of the weight-gradient slabs [chunk][tap][CoutPad][CinPad] into dW (torch layout)
void launch_wgrad_reduce(hipStream_t st, const float* ws, int chunks, int taps, int CoutPad, int CinPad, int Cout, int Cin,
                         float* dW, int accumulate);
// igemm.hip (C ABI): 1 when the forward / weight-gradient kernels take this shape with a consumer-side activation on the input
extern "C" int arco_conv_pro_ok(int taps, int NV, int D3, int H, int W, int Cin, int Cout, long ld_in, int mma, int groups);
