/* arco_hip.h - C ABI of libarco_hip.so: the MI355X (gfx950) kernels behind the ARCO
 * stratified pixel-contrastive training hot path.
 *
 * The reference (charlesyou999648/ARCO) is pure Python/PyTorch: it has no FFI layer, so the
 * "interface each entry point replaces" is the PyTorch call sequence at the cited reference
 * file:line (paths relative to the reference's code/ directory).  The Python host
 * (the modules of arco_amd) binds these with ctypes (arco_amd/_lib.py); INTEGRATION.md shows the stub.
 *
 * This file is the one definition of the ABI: it is compiled into every source of arco_amd/csrc (common.h includes it, so a
 * definition that disagrees with its declaration does not build), and arco_amd/_lib.py parses it at import into the ctypes
 * argtypes / restype of every entry point.  A new entry point is written twice - its definition and its declaration here -
 * and the compiler compares the two.  For the parser's sake a declaration is `<ret> arco_<name>(<params>);` with scalar
 * parameters of type int, long, float, double or uint64_t, anything else behind a pointer, and `void* stream` last where
 * the entry point enqueues work.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *    (PyTorch allocates), except the two host-side sampler entry points at the end;
 *  - no allocation, no ownership transfer, no global state: kernels are stateless, re-entrant,
 *    and are enqueued on the caller's HIP stream (`stream` = hipStream_t);
 *  - activations are channels-last fp32 "rows": pixel p of an [N, C, *spatial] tensor is the C
 *    consecutive floats at base + p*ld (ld >= C lets a channel slice be used in place);
 *  - return 0 on success, <0 on error (-1 bad argument, -2 launch failure, -3 unsupported);
 *    the *_ws_* / *_blocks / *_bytes helpers return sizes.
 */
#ifndef ARCO_HIP_H
#define ARCO_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- L1/L2  per-pixel class masks, counts, stable compaction (loss_helper_3d.py:341-342,352-358,
 *      364-401; loss_helper.py:512-572).  codes: bit c = low-valid, 21+c = anchor candidate,
 *      42+c = negative key (C <= 21).  totals = [n_low_valid[C] | n_anchor[C] | n_neg[C]].           */
int arco_mask_codes(const int64_t* lab_l, const int64_t* lab_u, const float* prob_l, const float* prob_u,
                    const float* low_mask, const float* high_mask, int n_l_img, int n_u_img, int C, long P,
                    float delta_p, float delta_n, int low_rank, int high_rank, uint64_t* codes,
                    uint32_t* block_counts, uint32_t* block_offsets, int64_t* totals, void* stream);
/* lists[(kind*C + c)*n_pix + j] = row id of the j-th anchor (kind 0) / negative (kind 1) pixel of class c,
 * in (b, spatial) row-major order == torch boolean-mask order (loss_helper_3d.py:377,403).                */
int arco_compact_rows(const uint64_t* codes, long n_pix, int C, const uint32_t* block_offsets, int32_t* lists,
                      void* stream);
/* prototype[c] = mean of teacher rows over low-valid pixels (loss_helper_3d.py:380-384); NaN when empty. */
long arco_proto_ws_floats(long n_pix, int C, int D);
int arco_masked_proto(const float* T, long ldt, const uint64_t* codes, long n_pix, int C, int D,
                      const int64_t* totals, float* partial, float* proto, void* stream);
/* linear-prototype path: low-valid bits as float rows; weighted row sums sum_rows Wt[row][c]*T[row][:]
 * (prototype = W_fea4 . masked mean of the fea4 INPUT, mask pushed through the bilinear adjoint)           */
int arco_lv_weights(const uint64_t* codes, long n_pix, int C, int Cp, float* W, void* stream);
int arco_weighted_row_sum(const float* T, long ldt, const float* Wt, long ldw, long n_rows, int C, int D,
                          const int64_t* totals, float* partial, float* out, long ldo, void* stream);
/* out[j] = src[list ? list[idx[j]] : idx[j]], idx = idx64 | idx32 | identity, j in [first, first+n)
 * (rep[mask][idx] / rep_teacher[negative_mask], loss_helper_3d.py:403,455-457).  D % 4 == 0: four elements per
 * access - ld_src and ld_out multiples of 4, src aligned to four elements, out to 16 bytes (else ARCO_ERR_ARG). */
int arco_gather_rows(const float* src, long ld_src, int D, const int32_t* list, const int64_t* idx64,
                     const int32_t* idx32, long first, long n, float* out, long ld_out, void* stream);
/* the same two with an f16 row matrix as the source (BASELINE.json configs[4], --act_dtype f16: the V-Net's full-resolution
 * feature maps are consumed by the heads as stored - FeatureExtractor_3d rows model_3D.py:52-58 - sums and rows are fp32)    */
int arco_weighted_row_sum_h(const void* T, long ldt, const float* Wt, long ldw, long n_rows, int C, int D,
                            const int64_t* totals, float* partial, float* out, long ldo, void* stream);
int arco_gather_rows_h(const void* src, long ld_src, int D, const int32_t* list, const int64_t* idx64,
                       const int32_t* idx32, long first, long n, float* out, long ld_out, void* stream);
/* ---- L3  out = cat(old, keys)[-min(len_old+n, queue_size):]  (dequeue_and_enqueue, loss_helper_3d.py:12-32) */
int arco_bank_append(const float* old, long len_old, const float* keys, long n, long queue_size, int D, float* out,
                     void* stream);
/* ---- L6  InfoNCE (loss_helper_3d.py:503-509): y = x/max(||x||,eps) (+transposed copy, +1/norm) ...      */
int arco_normalize_rows(const float* x, long ldx, long n, int D, float eps, float* y, long ldy, float* yt, long ldyt,
                        float* inv, void* stream);
/* ... M[q][k] = multiplicity of bank row k among query q's sampled negatives ...                          */
int arco_neg_multiplicity(const int64_t* idx, int Q, int Nn, long L, long ld, uint32_t* M, void* stream);
/* ... loss_q = logsumexp([pos, S[q, idx]]/T) - pos/T ; W = d loss_q/dS ; gpos = d loss_q/dpos             */
int arco_infonce_fwd(const float* S, long ld, const uint32_t* M, long L, const float* An, const float* Pn, long ldp,
                     int Q, int D, float temp, float* W, float* gpos, float* loss_q, void* stream);
/* ... dA = scale * d(loss)/dA through the cosine normalisation (G = W @ Bn)                                */
int arco_infonce_anchor_grad(const float* G, const float* An, const float* Pn, long ldp, const float* gpos,
                             const float* inv, int Q, int D, float eps, float scale, float* dA, void* stream);
/* ---- L5-L6 grouped: every class ("entry") of the per-class loop of loss_helper_3d.py:435-509 in ONE launch per stage.
   Host arrays of E <= 21 entries: banks[e] (device pointer of memobank[valid_classes[k]][0]), lens[e] (its rows),
   prow[e] (row of seg_proto[k] in the normalised prototype matrix), k[e] (loop counter = row-list index).              */
/* y = x / max(||x||, eps) written with zeroed pad columns [D, Dp) (anchors, prototypes)                                 */
int arco_normalize_rows_pad(const float* x, long ldx, long n, int D, int Dp, float eps, float* y, long ldy, float* inv,
                            void* stream);
/* Bn[E][Lp][Dp] = normalised bank rows (zero beyond lens[e] / D), Bt[E][Dp][Lp] = their transposes (nullable)          */
int arco_nce_normalize_banks(const void* const* banks, const int* lens, int E, int D, int Dp, long Lp, float eps, float* Bn,
                             float* Bt, void* stream);
/* batch independent GEMMs out_z = in_z . W_z^T (operand z at base + z*stride floats), optional split-K through ws:
   the cosine scores A_c . Bank_c^T (loss_helper_3d.py:503-505) and the anchor-gradient GEMMs W_c . Bank_c              */
int arco_gemm_batched(const float* in, long ld_in, int K, const float* Wp, int N, float* out, long ld_out, long M,
                      int batch, long stride_in, long stride_w, long stride_out, int splits, float* ws, void* stream);
/* per (query, entry): multiplicities of the sampled negatives (LDS), loss_q = logsumexp([pos, S[q, idx]]/T) - pos/T,
   W = d loss_q / dS over the whole padded row, gpos = d loss_q / d pos (loss_helper_3d.py:478-509)                      */
long arco_nce_max_len(void);
int arco_nce_fused(const float* S, long ld, const int* lens, const int* prow, int E, const int64_t* idx_all, long idx_off,
                   long idx_stride, int Q, int Nn, const float* An, const float* Pn_all, int Dp, float temp, float* W,
                   float* gpos, float* loss_q, void* stream);
/* dA[e*Q+q][0..D) = scale * d loss / d anchor through the cosine normalisation, all entries                            */
int arco_nce_anchor_grad(const float* G, const float* An, const float* Pn_all, const int* prow, int E, const float* gpos,
                         const float* inv, int Q, int D, int Dp, float eps, float scale, float* dA, long ld_dA, void* stream);
/* ---- L6, round 6: the score GEMM with the temperature-scaled softmax-CE in its EPILOGUE (north_star's wording; loss_helper_3d.py:503-509:
 *   logits = cat(pos, cosine(anchor, negatives)) / T; F.cross_entropy(logits, 0)) - no score matrix in HBM, the bank normalisation
 *   folded into the GEMM's B staging.  Five launches replace nine (2 x normalize_rows_pad, nce_normalize_banks, gemm_batched, nce_fused,
 *   sum_scale | gemm_batched + slab sum, nce_anchor_grad):
 *   arco_nce_prep    anchors / prototypes normalised (An, invA, Pn) + per (entry, query) the uint16 multiplicity row M[e*Q+q][0..Lp)
 *   arco_nce_score   S = An . bank^T on the matrix cores per (64 queries, 128 bank rows, entry); the B staging accumulates each bank
 *                    row's sum of squares; epilogue Wu = M * exp((cos - 1)/T) / ||b||, partial row sums Zp; pos = An . Pn[prow];
 *                    Bt = the raw bank transposed (the operand of the anchor-gradient GEMM)
 *   arco_nce_finish  loss_q = log Z - (pos - 1)/T with Z = sum Zp + exp((pos - 1)/T); gpos, gscale = 1/(T Z); the loss sum
 *   then arco_gemm_batched(Wu, Bt) and arco_nce_anchor_grad_scaled.  Same results as the staged route to fp32 rounding.         */
int arco_nce_prep(const float* A, long n_a, const float* P, long n_p, int D, int Dp, float eps, float* An, float* invA, float* Pn,
                  const int* lens, int E, const int64_t* idx_all, long idx_off, long idx_stride, int Q, int Nn, long Lp, void* M,
                  void* stream);
long arco_nce_score_ltiles(long Lp);
int arco_nce_score(const float* An, int Dp, int D, const void* const* banks, const int* lens, const int* prow, int E, long Lp, int Q,
                   const void* M, const float* Pn_all, float temp, float eps, float* Wu, float* Zp, float* pos, float* Bt, void* stream);
int arco_nce_finish(const float* pos, long n_rows, const float* Zp, long Lp, float temp, float scale, float* gpos, float* gscale,
                    float* loss_q, float* loss_sum, void* stream);
int arco_nce_anchor_grad_scaled(const float* Gu, const float* An, const float* Pn_all, const int* prow, int E, const float* gpos,
                                const float* inv, const float* gscale, int Q, int D, int Dp, float eps, float scale, float* dA, long ld_dA,
                                void* stream);
/* out[e*Q+q] = lists[k[e]][idx_all[e*idx_stride + q]]: pixel id of every sampled anchor (loss_helper_3d.py:455-457)     */
int arco_anchor_pix(const int32_t* lists, long n_pix, const int* k, int E, const int64_t* idx_all, long idx_stride, int Q,
                    int64_t* out, void* stream);
/* dst[list?list[idx[j]]:idx[j]] += alpha * (alpha_dev?*alpha_dev:1) * src[j]  (backward of the anchor gather) */
int arco_scatter_add_rows(const float* src, long ld_src, int D, const int32_t* list, const int64_t* idx, long n,
                          const float* alpha_dev, float alpha, float* dst, long ld_dst, void* stream);
int arco_sum_scale(const float* x, int n, float scale, float* out, int accumulate, void* stream);

/* 1 when a conv of this shape runs on the split-bf16 kernels (mma = 3: every fp32 operand = 3 bf16 terms, six bf16 MFMAs
   per 32 k, fp32-accurate) and therefore takes the split-packed weights (arco_pack_conv_weight mode | 2); else 0      */
int arco_conv_split_ok(int taps, int NB, int H, int W, int Cin, int Cout, long ld_in);
/* ---- N1-N4  convolutions on the fp32 matrix cores (nn.Conv2d 3x3 / 1x1: unetWithArgs.py:36-44,72,139;
 *      model_2D.py:25-33; train_arco_2d.py:231-234).  Wp = packed weights [taps][ceil16(N)][ceil16(K)].
 *      Sources: csrc/igemm.hip (forward / data gradient, weight packing, the shape queries), csrc/wgrad.hip (weight and bias
 *      gradients: arco_conv_wgrad, arco_conv3d_wgrad(_pro), arco_wgrad_*, arco_colsum(_h)), with the pipelined kernels of
 *      conv_sp.hip, conv3d_fl.hip and gemm_sp.hip behind the same entry points.                                */
int arco_pack_conv_weight(const float* W, int Cout, int Cin, int taps, int mode, float* Wp, void* stream);
/* all conv weights of a model in ONE launch: `desc` = device array of records {const float* src; float* dst;
 * int Cout, Cin, taps, mode, Npad, Kpad; long first;} (arco_pack_desc_bytes() bytes each).
 * mode bits: 1 data-gradient form (flipped + transposed), 2 split-bf16, 4 f16; mode >> 3 != 0 gathers the GEMM form of a
 * k2 s2 (transposed) convolution straight from the torch layout - nn.Conv3d(k2, s2) / nn.ConvTranspose3d(k2, s2) of
 * vnetWithArgs.py:67-118: 1 = W2[co][t*ci + c] = W[co][c][t], 2 = W2[t*co + o][ci] = W[ci][o][t], 4 = the bias repeated over
 * the 8 taps; `taps` then carries the inner dimension (ci resp. co), Cout / Cin are W2's logical [N][K]                */
long arco_pack_desc_bytes();
int arco_pack_many(const void* desc, int n_desc, long total, void* stream);
/* small-M x N, long-K GEMM (InfoNCE anchor gradient, loss_helper_3d.py:503-509 backward): K split into `splits`
 * slabs over grid.y, slab outputs in ws (splits*M*ld_out floats), fixed-order sum into out                  */
int arco_gemm_splitk(const float* in, long ld_in, int K, const float* Wp, int N, float* out, long ld_out, long M,
                     int splits, float* ws, void* stream);
int arco_conv_mblocks(int taps, int NB, int H, int W, int Cin, int Cout, long ld_in, int stat_groups);
int arco_conv_mblocks_mma(int taps, int NB, int H, int W, int Cin, int Cout, long ld_in, int stat_groups, int mma);   /* ... for a launch in matrix-core mode mma (arco_conv3d_fwd) */
int arco_conv_mblocks_pro(int taps, int NB, int H, int W, int Cin, int Cout, long ld_in, int stat_groups, int mma, int pro_groups);   /* ... for a launch through arco_conv3d_fwd_pro (3x3x3: the forms with the activation in their loaders tile differently) */
/* which kernel instantiation a launch uses: igemm_kernel<TAPS,BM,BN,..> -> TAPS*1e6 + BM*1e3 + BN;
 * conv3x3_halo_kernel<CIN,COUT,..> -> 9.9e6 + CIN*1e3 + COUT; conv3x3_image_kernel -> 9.8e6 + CIN*1e3 + 16; conv3d_image_kernel<DEPTH> ->
 * 9*DEPTH*1e6 + 701016; conv3d_rw16_kernel -> 9450016; the flat 3x3x3 igemm tiles add 5e5; conv_sp.hip / conv3d_fl.hip: see below.
 * Launch-only routes, which no query describes and only arco_conv_last_route reports:
 *   conv1x1_narrow_out_kernel<Q> -> 1.6e6 + K*1e3 + 4 (K = 4 Q = 4, 8, 16, 32: 1604004, 1608004, 1616004, 1632004)
 *   conv1x1_narrow_in_kernel     -> 1700000
 *   gemm_sp_kernel<false>        -> 1464256 (1e6 + 4e5 + BM*1e3 + BN, 64 x 256 tiles);  gemm_sp_kernel<true> (fused upsample) -> 1514256
 *   hconv1x1_narrow_out_kernel<Q> (mma 4) -> 1.8e6 + K*1e3 + 4 (K = 8 Q = 8, 16, 32: 1808004, 1816004, 1832004)
 *   hconv1x1_narrow_in_kernel     (mma 4) -> 1900000
 * The f16-storage kernels of conv_h.hip (mma 4): hconv_kernel<TAPS,BM,BN,..> -> TAPS*1e6 + BM*1e3 + BN with the kernel-tap form 9 for
 * 3x3 AND 3x3x3 (flat 3x3x3 tiles add 5e5), so the 2-D and the 3-D instantiation of one tile share an id and the `taps` argument of
 * the call tells them apart; hconv_rw_kernel<1,1,8> -> 9408016; hconv_fc_kernel<A_T,C_T> -> 9.26e6 + A_T*1e3 + 16 C_T. */
int arco_conv_config(int taps, int NB, int H, int W, int Cin, int Cout, long ld_in, int* kc_depth_db);
int arco_conv_config_mma(int taps, int NB, int H, int W, int Cin, int Cout, long ld_in, int mma);
/* test-facing: the id, as above, of the kernel that the most recent forward launch on the calling thread took (arco_conv_fwd,
 * arco_conv3d_fwd(_pro), arco_gemm_splitk, arco_gemm_batched, arco_conv1x1_upres_fwd).  Each of these sets it to 0 once its arguments
 * have passed: it is 0 before the first launch, after a call that found no kernel (ARCO_ERR_UNSUPPORTED, such as a refused
 * arco_conv1x1_upres_fwd).  The kernels of conv_h.hip (mma 4) note their ids too (listed above; the two streaming kernels are
 * launch-only); the one-channel 3x3x3 volume runs on conv3d_image_kernel<3> in mma 4 as well and reports 27701016.  A call rejected
 * with ARCO_ERR_ARG - the pointer-alignment checks of mma 4 included - leaves it unchanged.
 * Host side only: nothing on the device changes. */
int arco_conv_last_route(void);
/* A/B switch of the software-pipelined split-bf16 3x3 kernel (conv_sp.hip; ids 9.3e6 + A_T*1e3 + BN, resident-weights form 9.35e6 + ...): on = 1
 * (default) lets the eligible wide 2-D shapes take it, 0 keeps every shape on
 * igemm_kernel.  Returns the previous setting.  Tile counts differ: query arco_conv_mblocks_mma after switching.   */
int arco_conv_sp_set(int on);
/* A/B switch of the software-pipelined flat-tile 3x3x3 kernel (conv3d_fl.hip; ids 9.27e6 / 9.29e6 + A_T*1e3 + BN for its per-step and per-chunk forms: the 32 .. 256-channel levels of
 * the V-Net, vnetWithArgs.py:5-31): on = 0 keeps every 3x3x3 launch on igemm_kernel.  Outputs are bit-identical
 * either way; tile counts differ (query arco_conv_mblocks_mma after switching).  Returns the previous setting. */
int arco_conv3d_fl_set(int on);
/* A/B switch of the software-pipelined split-bf16 1x1 GEMM (gemm_sp.hip; the wide many-tile FeatureExtractor / q_representation GEMMs,
 * model_2D.py:20-55, train_arco_2d.py:231-234): on = 0 keeps every GEMM on igemm_kernel; min_tiles > 0 also sets the
 * smallest 128 x 128 tile count the kernel takes (default 2048).  Outputs are bit-identical either way.  Returns the
 * previous `on`. */
int arco_gemm_sp_set(int on, long min_tiles);
/* out = W . in + trilinear_align_corners(lo): the 1x1x1 conv over a high-resolution feature map with the upsampled low-resolution
 * product as residual, sampled in the GEMM's epilogue (FeatureExtractor_3d, model_3D.py:46-58: `fea_i(cat(up(x), f_i)) + cat(...)` with
 * the wide weight block evaluated below the upsample).  Wp: split-bf16 pack.  Returns ARCO_ERR_UNSUPPORTED (-3) when the pipelined
 * kernel does not take the shape - the caller then upsamples with arco_trilinear_fwd and passes the result as arco_conv3d_fwd's residual;
 * both routes give bit-identical outputs. */
int arco_conv1x1_upres_fwd(const float* in, long ld_in, int K, const float* Wp, int N, float* out, long ld_out, const float* lo,
                           long ld_lo, int NV, int uD, int uH, int uW, int oD, int oH, int oW, void* stream);
/* out = conv(in) (+bias)(+residual); optional per-channel (sum, sumsq) block partials for train-mode BN. */
int arco_conv_fwd(const float* in, long ld_in, int K, const float* Wp, int N, float* out, long ld_out,
                  const float* bias, const float* residual, long ld_res, float* stat_sum, float* stat_sq, int taps,
                  int NB, int H, int W, void* stream);
/* 3-D: NV volumes of D3 planes of H x W; taps = 27 is nn.Conv3d(3, padding=1) (vnetWithArgs.py:16)      */
int arco_conv3d_fwd(const float* in, long ld_in, int K, const float* Wp, int N, float* out, long ld_out,
                    const float* bias, const float* residual, long ld_res, float* stat_sum, float* stat_sq, int taps,
                    int NV, int D3, int H, int W,
                    int stat_groups /* BN groups: volumes [g*NV/G,..) feed stat slabs [g*nmb/G,..); 1 = one batch */, int mma /* 0: fp32 MFMA (default, parity); 1 / 2: the operands of the 3x3x3 convolutions and 1x1x1 GEMMs
                               rounded to f16 / bf16 in registers (BASELINE.json configs[4] "fp16 MFMA conv"; tolerance 1e-2; opt-in), on
                               the plain fp32 pack (mode 0 / 1).  Contract, held bit for bit by tests/test_mma12_kernels_gpu.py: BOTH
                               operands rounded to nearest even - f16 with gradual underflow (subnormal operands are kept) and overflow
                               to +-inf (65520 and above become infinity, not 65504; inf * 0 = NaN follows) -, the products exact (22 /
                               16 bits), fp32 accumulation, bias and residual unrounded in the fp32 epilogue: the result is the fp32
                               convolution of the rounded operands.  Shapes that run the fp32 arithmetic of mma 0 whatever the mode: taps
                               9 (3x3 per plane, any D3), K % 4 != 0 or ld_in % 4 != 0 (the scalar-load form), the one-channel 3x3x3
                               volume (conv3d_image_kernel<3>); the streaming 1x1 kernels are not taken in these modes. 3: split-bf16
                               (the mode | 2 pack); 4: f16 activation storage (conv_h.hip, the mode | 4 pack) */,
                    void* stream);
int arco_conv3d_wgrad(const float* dZ, long ld_dz, int Cout, const float* in, long ld_in, int Cin, int taps, int NV,
                      int D3, int H, int W, float* ws, float* dW, int accumulate,
                      int mma /* 0 exact fp32; != 0: 3x3x3 halo kernels with bf16 MFMA operands, fp32 accumulate */, void* stream);
long arco_wgrad_ws_floats(int Cout, int Cin, int taps, long M);
/* which weight-gradient kernel a launch uses, decided by the host function that the launch itself calls.  entry 0: arco_conv_wgrad /
 * arco_conv3d_wgrad (pro_groups = 0) / arco_conv3d_wgrad_pro (pro_groups = its BatchNorm groups >= 1); entry 1:
 * arco_conv3x3_image_wgrad_h (taps 9, D3 1, Cin = its K).  aligned16: dZ and `in` start on 16-byte boundaries.  Returns the id or
 * ARCO_ERR_UNSUPPORTED (-3) where the launch would; *slabs = slabs written to ws (= workgroups along x, never more than
 * arco_wgrad_ws_floats reserves for the same Cout, Cin, taps, M), *slab_floats = floats per slab, *reduce = the slab sum that follows:
 * 1 wgrad_reduce_kernel<64,8>, 2 wgrad_reduce_kernel<16,32>, 3 wgrad_reduce4_kernel.  The three pointers may be NULL.
 * mma 4 with Cin = 1 and taps >= 9 (f16 dZ against the fp32 one-channel volume) exists on wgrad_image3d_kernel only (Cout in 4, 8, 12,
 * 16 and ld_dz a multiple of 4): any other such shape is ARCO_ERR_UNSUPPORTED, in the query and in the launch.
 * Ids: T*1e6 + F*1e5 + V*1e4 + COB*100 + CIB, T = 1 (taps 1) or 9 (taps 9 and 27), COB x CIB the channel tile:
 *   F 0  wgrad_kernel<COB,CIB>                  1001616 .. 1006464
 *   F 1  wgrad_q_kernel<64>                     1100064 (the pixels per staged tile in the CIB field)
 *   F 2  wgrad_halo2_kernel<COB,CIB,FLAT,MODE>  V = FLAT + 2 * (bf16 operands): 9201616 rectangular fp32, 9211616 flat fp32, 9221616, 9231616
 *   F 3  wgrad_split_kernel<COB,CIB,PRO>        V = PRO: 9301616 .. 9303232, 9311616 .. 9313232
 *   F 4  wgrad_image3d_kernel<DEPTH>            V = DEPTH: 9411616, 9431616
 *   F 5  hwgrad_kernel<COB/16,CIB/16,NT>        T = NT: 9501616 .. 9503232, 1501616 .. 1506464
 *   F 6  himage_wgrad_kernel                    9601600 + K: 9601601 .. 9601604                                                    */
int arco_wgrad_config(int entry, int taps, int NV, int D3, int H, int W, int Cin, int Cout, long ld_dz, long ld_in, int mma,
                      int pro_groups, int aligned16, long* slabs, long* slab_floats, int* reduce);
/* test-facing: the id, as above, of the kernel that the most recent weight-gradient launch on the calling thread took (arco_conv_wgrad,
 * arco_conv3d_wgrad(_pro), arco_conv3x3_image_wgrad_h; the f16 kernels of mma 4 included).  0 before the first launch and after a call
 * that found no kernel (ARCO_ERR_UNSUPPORTED); a call rejected with ARCO_ERR_ARG leaves it unchanged.  Host side only. */
int arco_wgrad_last_route(void);

/* ---- Consumer-side activation: a block's first Conv-BN-LeakyReLU-Dropout stage (unetWithArgs.py:36-44: conv_conv[0..3]) without the
 * BatchNorm-apply pass.  The producing convolution writes its PRE-activation z (and the BN partial statistics); the block's second
 * convolution - and, in the backward pass, the weight gradient of that second convolution - form
 *     a = dropout(lrelu((z - mean) * istd * gamma + beta))
 * element by element in their loaders while they stage z for the matrix cores (conv_sp.hip producer waves, wgrad_split_kernel): the
 * activation never exists in HBM (2 of the 4 HBM crossings of every such activation, and one launch per stage, are gone).  The
 * arithmetic is arco_bn_act_fwd's operation for operation: results are bit-identical to the two-pass route.
 * The struct below is the kernels' own definition (csrc/igemm_args.h asserts its 64 bytes, seed at 48); arco_amd/_lib.py ActPro
 * mirrors it field for field.                                                                                                      */
typedef struct ArcoActPro {
  const float* mean; const float* istd;   /* [groups][K] batch statistics of the producing layer (arco_bn_finalize)                 */
  const float* gamma; const float* beta;  /* [K] nn.BatchNorm2d weight / bias                                                       */
  float slope;                            /* nn.LeakyReLU negative_slope (0: ReLU)                                                   */
  int groups;                             /* BatchNorm groups: images [g*NV/G, (g+1)*NV/G) use statistics row g                     */
  int drop_mode; float p;                 /* 0: none; 1: nn.Dropout(p), the stateless mask of arco_bn_act_fwd (element = pixel*K + k) */
  unsigned long long seed; const unsigned long long* seed_dev;   /* as arco_bn_act_fwd (seed_dev: per-replay salt of a HIP graph)    */
} ArcoActPro;
/* 1 when the entry points below take the shape (taps = 9: 3x3, split-bf16 mode 3, the pipelined kernels - forward and weight gradient;
 * taps = 27: the V-Net's 3x3x3 stage -> stage links (vnetWithArgs.py:5-31; conv3d_fc_kernel's loaders, BatchNorm + ReLU, no dropout) -
 * FORWARD ONLY, for gradient-free passes, with the BatchNorm slab count from arco_conv_mblocks_pro); else the caller runs
 * arco_bn_act_fwd and the plain entry points */
int arco_conv_pro_ok(int taps, int NV, int D3, int H, int W, int Cin, int Cout, long ld_in, int mma, int groups);
int arco_conv3d_fwd_pro(const float* z_in, long ld_in, int K, const float* Wp, int N, float* out, long ld_out,
                        const float* bias, const float* residual, long ld_res, float* stat_sum, float* stat_sq, int taps,
                        int NV, int D3, int H, int W, int stat_groups, int mma, const ArcoActPro* pro, void* stream);
int arco_conv3d_wgrad_pro(const float* dZ, long ld_dz, int Cout, const float* z_in, long ld_in, int Cin, int taps, int NV,
                          int D3, int H, int W, float* ws, float* dW, int accumulate, int mma, const ArcoActPro* pro, void* stream);
/* dW[co][ci][tap] (+)= sum_pix dZ[pix][co] * in[pix+tap][ci]   (torch weight layout)                      */
int arco_conv_wgrad(const float* dZ, long ld_dz, int Cout, const float* in, long ld_in, int Cin, int taps, int NB,
                    int H, int W, float* ws, float* dW, int accumulate, void* stream);
int arco_colsum(const float* X, long ldx, long M, int C, float* ws, float* out, int accumulate, void* stream);
int arco_transpose2d(const float* x, long ldx, int rows, int cols, float* y, long ldy, void* stream);

/* ---- N1  train-mode BatchNorm + (Leaky)ReLU + dropout (nn.BatchNorm2d/LeakyReLU/Dropout,
 *      unetWithArgs.py:36-44; vnetWithArgs.py:16-25)                                                      */
int arco_bn_finalize(const float* ssum, const float* ssq, int nblk, int C, long count, float eps, float momentum,
                     float* mean, float* istd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                     int groups /* mean/istd rows: [groups][C] */,
                     int defer_from, float* deferred /* nullable: groups >= defer_from postpone their running-statistics
                     update into deferred[groups - defer_from][2][C] (+1 flag float), see arco_bn_apply_deferred */,
                     void* stream);
/*      postponed momentum updates of many BN layers, one launch: desc = device array of n_layers records
 *      {float* running_mean, running_var, deferred; int C, n; float momentum; int pad} (arco_bn_defer_desc_bytes() each).
 *      The reference runs model(l), model(cj2_l), model(u) (train_arco_2d.py:310-312); the build runs (l, u) as one
 *      grouped pass and cj2_l afterwards - the running statistics must still receive the updates in the reference's order */
long arco_bn_defer_desc_bytes(void);
int arco_bn_apply_deferred(const void* desc, int n_layers, void* stream);
int arco_chan_stats_blocks(long M);
int arco_chan_stats(const float* X, long ldx, long M, int C, float* ssum, float* ssq, int groups, void* stream);
int arco_bn_act_fwd(const float* Z, long ldz, long M, int C, const float* mean, const float* istd, const float* gamma,
                    const float* beta, float slope, int drop_mode, float p, uint64_t seed, long P, float* A, long lda,
                    const uint64_t* seed_dev, int groups, void* stream);
int arco_bn_act_bwd(const float* dA, long ldd, const float* Z, long ldz, long M, int C, const float* mean,
                    const float* istd, const float* gamma, const float* beta, float slope, int drop_mode, float p,
                    uint64_t seed, long P, float* ws, float* dgamma, float* dbeta, int accumulate, float* dZ, long ldo,
                    const uint64_t* seed_dev /* same device salt as the forward (graph replays), or NULL */, int groups, void* stream);
/* ---- N2/N3  nn.MaxPool2d(2) (unetWithArgs.py:55-58); nn.Upsample(bilinear, align_corners=True)
 *      (unetWithArgs.py:74-75, model_2D.py:43-52)                                                          */
/* GroupNorm / InstanceNorm + ReLU of the V-Net blocks (vnetWithArgs.py:19-22,48-51,76-79 `normalization='groupnorm'` =
 * nn.GroupNorm(16, C), `'instancenorm'` = nn.InstanceNorm3d(C)): statistics per sample over a set of cpg channels.
 * Forward: arco_chan_stats(groups = N) -> arco_gn_finalize -> arco_bn_act_fwd(groups = N) (mean / istd rows [N][C]);
 * backward: arco_gn_act_bwd (ws as for arco_bn_act_bwd with groups = N)                                                */
int arco_gn_finalize(const float* ssum, const float* ssq, int nblk, int C, int cpg, int N, long count_per_sample_channel,
                     float eps, float* mean, float* istd, void* stream);
int arco_gn_act_bwd(const float* dA, long ldd, const float* Z, long ldz, long M, int C, const float* mean,
                    const float* istd, const float* gamma, const float* beta, float slope, float* ws, float* dgamma,
                    float* dbeta, int accumulate, float* dZ, long ldo, int N, int cpg, void* stream);
int arco_maxpool2_fwd(const float* X, long ldx, int NB, int H, int W, int C, float* Y, long ldy, void* stream);
/* A = lrelu(BN(Z)) (mean / istd rows [groups][C] as arco_bn_act_fwd, no dropout) and P = maxpool2(A) in one pass: the last
   stage of a ConvBlock whose output feeds the next DownBlock's nn.MaxPool2d and the decoder's skip (unetWithArgs.py:36-44,
   55-58,109-116)                                                                                              */
int arco_bn_act_pool_fwd(const float* Z, long ldz, int NB, int H, int W, int C, const float* mean, const float* istd,
                         const float* gamma, const float* beta, float slope, float* A, long lda, float* P, long ldp,
                         int groups, void* stream);
int arco_maxpool2_bwd(const float* X, long ldx, int NB, int H, int W, int C, const float* dY, long ldy, float* dX,
                      long ldo, void* stream);
/* ... fused with the gradient x receives from its second consumer (unetWithArgs.py:109-116,142-158: x_i feeds both the
   next DownBlock and the decoder's skip concat): dX = maxpool2_bwd(dY) + add                                          */
int arco_maxpool2_bwd_add(const float* X, long ldx, int NB, int H, int W, int C, const float* dY, long ldy, const float* add,
                          long ld_add, float* dX, long ldo, void* stream);
int arco_bilinear_fwd(const float* X, long ldx, int NB, int Hi, int Wi, int C, int Ho, int Wo, float* Y, long ldy,
                      void* stream);
int arco_bilinear_bwd(const float* dY, long ldy, int NB, int Hi, int Wi, int C, int Ho, int Wo, float* dX, long ldx,
                      int accumulate, void* stream);
/* rows of cat(upsample(lo), hi) at selected high-res pixels, and the adjoint scatter (row-sparse head of
 * FeatureExtractor.fea4 / q_representation: model_2D.py:51-53, train_arco_2d.py:324-325)                   */
int arco_gather_upcat_rows(const float* lo, long ldlo, int Clo, int Hi, int Wi, const float* hi, long ldhi, int Chi,
                           int Ho, int Wo, const int64_t* pix, long n, float* X, long ldx, void* stream);
/* (arco_scatter_upcat_rows: fp32 atomics, no alignment requirement; ARCO_ERR_ARG for n < 0, a negative channel count, a size <= 0 or,
 * when n > 0, a null dX / pix / dlo (Clo > 0) / dhi (Chi > 0).  n == 0 returns ARCO_OK before any pointer is looked at, here and in
 * every row kernel below.)                                                                                  */
int arco_scatter_upcat_rows(const float* dX, long ldx, const int64_t* pix, long n, float* dlo, long ldlo, int Clo,
                            int Hi, int Wi, float* dhi, long ldhi, int Chi, int Ho, int Wo, void* stream);
/* second level of the row-sparse head: explicit low-res neighbour rows of each anchor (ids + (ly,lx)),
 * their 4-way lerp + cat with the high-res map, and the adjoint                                            */
/* (arco_up_neighbors rejects n < 0, a size <= 0 and null pointers; arco_lerp4_cat_rows_bwd also dX / dV that are not 16-byte
 * aligned - it moves four channels at a time -, dV may be null only with Clo == 0, dhi only with Chi == 0) */
int arco_up_neighbors(const int64_t* pix, long n, int Hi, int Wi, int Ho, int Wo, int64_t* nb4, float* lylx, void* stream);
int arco_lerp4_cat_rows(const float* V, long ldv, int Clo, const float* lylx, const float* hi, long ldhi, int Chi,
                        const int64_t* pix, long n, float* X, long ldx, void* stream);
int arco_lerp4_cat_rows_bwd(const float* dX, long ldx, int Clo, const float* lylx, const int64_t* pix, long n, float* dV,
                            long ldv, float* dhi, long ldhi, int Chi, void* stream);
/* ... with the map `hi` stored as f16 (f16 activation storage of the U-Net, train_arco_2d --fm_rows f16): ldhi in f16 elements,
 * Chi % 4 == 0, ldhi >= Chi; lo / V and X fp32.  The f16 values are widened exactly, so X equals what the fp32 entry point
 * returns on the upcast map bit for bit.  The adjoints keep fp32 targets (arco_cast_rows_f2h rounds the touched rows once).  */
int arco_gather_upcat_rows_h(const float* lo, long ldlo, int Clo, int Hi, int Wi, const void* hi, long ldhi, int Chi,
                             int Ho, int Wo, const int64_t* pix, long n, float* X, long ldx, void* stream);
int arco_lerp4_cat_rows_h(const float* V, long ldv, int Clo, const float* lylx, const void* hi, long ldhi, int Chi,
                          const int64_t* pix, long n, float* X, long ldx, void* stream);
/* V-Net k2s2 (transposed) convs as GEMMs over packed 2x2x2 blocks (vnetWithArgs.py:67-118); trilinear
 * align_corners resize of FeatureExtractor_3d (model_3D.py:46-58).
 * All three move four channels (16 bytes) per access: C and the strides are multiples of 4, the base pointers 16-byte aligned, every
 * size positive, dir 0 or 1 - anything else is ARCO_ERR_ARG before a launch.                                */
int arco_s2d3(float* V, long ldv, int NV, int X2, int Y2, int Z2, int C, float* P, long ldp, int dir, void* stream);
int arco_trilinear_fwd(const float* X, long ldx, int NV, int Di, int Hi, int Wi, int C, int Do, int Ho, int Wo, float* Y,
                       long ldy, void* stream);
int arco_trilinear_bwd(const float* dY, long ldy, int NV, int Di, int Hi, int Wi, int C, int Do, int Ho, int Wo, float* dX,
                       long ldx, void* stream);
/* 3-D row-sparse head: rows of cat(trilinear_up(lo), hi) at selected voxels + adjoint (model_3D.py:52-55).
 * The gathers (and arco_lerp8_cat_rows3d / arco_lerp8_rows3d_bwd below) move four channels per access: channel counts and strides are
 * multiples of 4, lo / V / X / dX / dV 16-byte aligned, hi 16-byte (f16: 8-byte) aligned; sizes positive, n >= 0, channel counts >= 0;
 * lo may be null only with Clo == 0, hi only with Chi == 0 (an operand of no channels is never read: neither its pointer nor its
 * alignment is looked at).  The scatter uses scalar fp32 atomics: the null and size checks only.                                  */
int arco_gather_upcat_rows3d(const float* lo, long ldlo, int Clo, int Di, int Hi, int Wi, const float* hi, long ldhi, int Chi,
                             int Do, int Ho, int Wo, const int64_t* pix, long n, float* X, long ldx, void* stream);
int arco_scatter_upcat_rows3d(const float* dX, long ldx, const int64_t* pix, long n, float* dlo, long ldlo, int Clo, int Di,
                              int Hi, int Wi, float* dhi, long ldhi, int Chi, int Do, int Ho, int Wo, void* stream);
/* ... with `hi` stored as f16; and the way back for its row-sparse gradient: rows idx[] of an fp32 buffer -> the same rows of an
 * f16 buffer, times the loss scale, saturated at +-65504 (arco_cast_f2h on the touched rows only); arco_zero_rows for f16       */
int arco_gather_upcat_rows3d_h(const float* lo, long ldlo, int Clo, int Di, int Hi, int Wi, const void* hi, long ldhi, int Chi,
                               int Do, int Ho, int Wo, const int64_t* pix, long n, float* X, long ldx, void* stream);
/* The level below evaluated lazily too (arco_amd/head.py LazyHead3dL3Fn; model_3D.py:46-58 one level further down): V = the eight
 * corner rows (8 j + k, arco_corner_rows3d's order) of every sampled voxel, each already through its own layer; X[j] = cat(their
 * trilinear blend in the gather's arithmetic, hi[pix[j]]); _bwd: dV[8 j + k] = w8[8 j + k] * dX[j][0..Clo)                        */
int arco_lerp8_cat_rows3d(const float* V, long ldv, int Clo, int Di, int Hi, int Wi, const float* hi, long ldhi, int Chi,
                          int Do, int Ho, int Wo, const int64_t* pix, long n, float* X, long ldx, void* stream);
int arco_lerp8_cat_rows3d_h(const float* V, long ldv, int Clo, int Di, int Hi, int Wi, const void* hi, long ldhi, int Chi,
                            int Do, int Ho, int Wo, const int64_t* pix, long n, float* X, long ldx, void* stream);
int arco_lerp8_rows3d_bwd(const float* dX, long ldx, int Clo, const float* w8, long n, float* dV, long ldv, void* stream);
int arco_cast_rows_f2h(const float* src, long ld_src, int C, const int64_t* idx, long n, float scale, void* dst, long ld_dst,
                       void* stream);
int arco_zero_rows_h(void* dst, long ld, int C, const int64_t* idx, long n, void* stream);
/* Order-independent form of the row-scatter adjoints above (csrc/det_scatter.hip): fp32 atomics sum in arrival order (one ulp of
 * run-to-run difference, as in torch's own upsample backward on the GPU that the reference runs: model_3D.py:52-55); these
 * accumulate fixed-point int64 (2^44 units for the largest |source element|, arco_det_absmax) - bit-reproducible.
 *   arco_det_absmax:        maxbits[0] = max bits(|X[r][c]|) over [n, C]  (>= 0x7f800000: a non-finite element)
 *   arco_det_scatter_rows:  acc[r(e)][c] += fix(w[e] * src[e / div][c]),  r(e) = list ? list[idx[e]] : idx[e],  e < n_e  (w nullable = 1)
 *   arco_det_finish_rows:   dst[r(e)][c]  = alpha * fp32(acc[r(e)][c])    (nan when the source was non-finite)
 *   arco_det_clear_rows:    acc[r(e)][c]  = 0                             (acc: persistent, zero between uses)
 *   arco_corner_rows3d:     idx8[8j+k], w8[8j+k] = low-resolution row and weight of corner k of sampled voxel pix[j]
 * An all-zero source (maxbits[0] == 0): arco_det_scatter_rows adds nothing and arco_det_finish_rows WRITES NOTHING - dst keeps what it
 * held, so a caller that needs zeros there fills them itself (arco_amd/head.py does).  A non-finite source: nothing is accumulated
 * and finish writes the quiet NaN 0x7fc00000 into every named row.
 * Arguments: n / n_e / M < 0, C <= 0, div < 1 and a null pointer (list and w excepted) are ARCO_ERR_ARG before any launch; acc is
 * 8-byte aligned.  n_e == 0 (arco_corner_rows*: n == 0) is a no-op that returns ARCO_OK; arco_det_absmax with n == 0 still sets
 * maxbits[0] = 0.                                                                                                                  */
int arco_det_absmax(const float* X, long ld, int C, long n, unsigned* maxbits, void* stream);
int arco_det_scatter_rows(const float* src, long ld_src, int C, int div, const int32_t* list, const int64_t* idx, const float* w,
                          long n_e, long long* acc, long ld_acc, const unsigned* maxbits, void* stream);
int arco_det_finish_rows(const int32_t* list, const int64_t* idx, long n_e, const long long* acc, long ld_acc, int C,
                         const unsigned* maxbits, float alpha, float* dst, long ld_dst, void* stream);
int arco_det_clear_rows(const int32_t* list, const int64_t* idx, long n_e, long long* acc, long ld_acc, int C, void* stream);
int arco_corner_rows3d(const int64_t* pix, long n, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int64_t* idx8, float* w8,
                       void* stream);
/*   arco_corner_rows2d:     the bilinear counterpart (four corners; adjoint of arco_gather_upcat_rows, model_2D.py:43-50)              */
int arco_corner_rows2d(const int64_t* pix, long n, int Hi, int Wi, int Ho, int Wo, int64_t* idx4, float* w4, void* stream);
/* Row-sparse backward of the dense per-pixel layers (nn.Conv2d(k=1) of FeatureExtractor / q_representation called on whole maps:
 * model_2D.py:51-53, train_arco_2d.py:231-234, 324-326).  The loss reads `rep` at a few hundred sampled rows (loss_helper_3d.py:455-457),
 * so d loss / d rep - and, the layers being per-pixel, every gradient down to the first resampling - is zero in all other rows:
 *   arco_row_nonzero: flag[r] = any element of row r that is not +-0   (one pass over the gradient)
 *   arco_put_rows:    dst[idx[j]] = src[j]  (idx unique: the compacted data gradient back into a zero tensor)
 * Both read four channels at a time: strides multiples of 4, X / src / dst 16-byte aligned; M / n < 0 is ARCO_ERR_ARG, 0 a no-op.       */
int arco_row_nonzero(const float* X, long ld, int C, long M, unsigned char* flag, void* stream);
int arco_put_rows(const float* src, long ld_src, int C, const int64_t* idx, long n, float* dst, long ld_dst, void* stream);
/* glue kernels replacing chains of tensor-library launches in the step (no reference counterpart: the reference's
 * autograd does these as separate zeros / add / copy / mul kernels, train_arco_2d.py:426-431, model_2D.py:43-50):
 * arco_zero_rows: rows idx[] of a [rows, ld] buffer zeroed over C channels (re-arms a persistent gradient buffer);
 * arco_fold_residual / arco_unfold_residual: W' = W + I split into its column blocks [n, c] | [n, n - c], and the gradient back;
 * arco_combine_terms(_bwd): out = sum_i w_i * term_i over <= 8 device scalars (host arrays of pointers / weights), grads_i = w_i * g */
int arco_zero_rows(float* dst, long ld, int C, const int64_t* idx, long n, void* stream);
int arco_fold_residual(const float* W, int n, int c, float* lo, float* hi, void* stream);
int arco_unfold_residual(const float* dlo, const float* dhi, int n, int c, float* dW, void* stream);
int arco_combine_terms(const float* const* terms, const float* weights, int n, float* out, void* stream);
int arco_combine_terms_bwd(const float* weights, int n, const float* g, float* grads, void* stream);
/* arco_copy_rows: C and the strides multiples of 4, X / Y non-null and 16-byte aligned, M >= 0 (0: nothing to do), C > 0.
 * The layout transposes: non-null pointers, P > 0, C > 0, NB in 1 .. 65535 (the grid's z extent).                        */
int arco_copy_rows(const float* X, long ldx, long M, int C, float* Y, long ldy, int accumulate, void* stream);
int arco_nchw_to_nhwc(const float* X, int NB, int C, long P, float* Y, long ldy, void* stream);
int arco_nhwc_to_nchw(const float* X, long ldx, int NB, int C, long P, float* Y, void* stream);

/* ---- O1/N5  torch.optim.SGD(nesterov) step and EMA over flat buffers (train_arco_2d.py:248,306-308,431-432;
 *      model_2D.py:176-182)                                                                                */
/* (n < 0 and, for n > 0, null pointers are ARCO_ERR_ARG; n == 0 does nothing - arco_sgd_momentum and arco_ema alike) */
int arco_sgd_nesterov(float* p, const float* g, float* buf, long n, float lr, float momentum, float weight_decay,
                      int first, void* stream);
/* the same with nesterov=False (stage-1 pre-training: pretrain_2D.py:193-195, pretrain_3D.py) */
int arco_sgd_momentum(float* p, const float* g, float* buf, long n, float lr, float momentum, float weight_decay,
                      int first, void* stream);
int arco_ema(float* k, const float* q, long n, float m, void* stream);

/* ---- T1  trainer glue (train_arco_2d.py:284-286,342-393,492-498)                                        */
int arco_softmax_rows(const float* X, long ld, long M, int C, long P, float* prob_planes, float* maxp, int64_t* amax,
                      float* entropy, void* stream);
int arco_label_onehot(const int64_t* lab, long M, int C, long P, int64_t* out, void* stream);
/* ---- §8f row 1: supervised CrossEntropy + Dice (train_arco_2d.py:336-339, utils/losses.py:173-209) and the
 *      confidence-weighted unsupervised CE (train_arco_2d.py:482-489) on channels-last logits             */
/* ---- E  equivariance loss (train_arco_2d.py:404-423; tps/rand_tps.py, tps_stn_pytorch/tps_grid_gen.py:59-71,
 *      tps/grid_sample.py:11-12 = F.grid_sample(bilinear, align_corners=True))                                  */
int arco_tps_grid(const float* rep, const float* mapping, int B, long HW, int NR, float* grid, void* stream);
int arco_grid_sample_fwd(const float* X, long ldx, int NB, int H, int W, int D3 /* slices per volume, 1 in 2-D */, int C,
                         const float* grid, int Ho, int Wo, int border, float* Y, long ldy, void* stream);
/* ---- A3 photometric augmentation of batch_transform (augment.py:148-225, 255-281): Pillow's 8-bit integer arithmetic
   (to_pil_image quantisation, ImageEnhance blends of torchvision's ColorJitter in fn_idx order, convert L / HSV,
   ImagingGaussianBlur = 3 box passes per direction, to_tensor).  data / out [B,C,H,W] fp32, C = 1 or 3, B <= 32;
   desc: HOST array of B records {int order[4]; float f[4]; int jitter, blur; float blur_r;} (arco_jitter_desc_bytes() each);
   ws: B uint64 + B*C*H*W floats.  arco_quantize8: floor(x*255)/255 (the confidence map's PIL round trip).               */
long arco_jitter_desc_bytes(void);
int arco_jitter_blur(const float* data, int B, int C, int H, int W, const void* desc_host, void* ws, float* out, void* stream);
int arco_quantize8(const float* x, long n, float* out, void* stream);
/* ---- A2 AdvMorph (adv_morph.py:310-580): 2-channel fields kept channels-last [B,H,W,2] (a field is a grid_sample grid;
   applyComposition2D = arco_grid_sample_fwd with border padding).  out = alpha*in + beta*base_grid (get_base_grid, :184-207),
   optional clamp to [-1,1]; depthwise ks x ks filter with zero padding (gaussian_smooth, :445-497; weights: host array);
   F.interpolate(bilinear, align_corners=False) (:507-508)                                                              */
int arco_field_axpb(const float* in, float alpha, float beta, const float* in2, float gamma, int B, int H, int W, int clamp,
                    float* out, void* stream);   /* out = alpha*in + beta*base_grid + gamma*in2 */
int arco_field_smooth(const float* in, int B, int H, int W, int C, int ks, const float* weights_host, float* out, void* stream);
int arco_field_resize(const float* in, int B, int h, int w, int C, int H, int W, float* out, void* stream);
int arco_eqv_loss_fwd(const float* P_, long ldp, const float* Q_, long ldq, const float* mask, int B, long P, int C, double* ws,
                      float* out, void* stream);
int arco_eqv_loss_bwd(const float* P_, long ldp, const float* Q_, long ldq, const float* mask, int B, long P, int C,
                      const double* ws, const float* g, float* dP, long ldo, void* stream);
/* ---- V  evaluation (test_2D.py:52-66): out[c] = {|pred==c|, |gt==c|, |pred==c & gt==c|} as int64[C][3]          */
int arco_overlap_counts(const int64_t* pred, const int64_t* gt, long n, int C, int64_t* out, void* stream);
/* ---- V  exact surface distances behind hd95 / asd (medpy.metric.binary with unit voxel spacing and connectivity 1, test_2D.py:52-66,
 *      test_util.py:214-220) of two contiguous label volumes [D][H][W], for every class c_lo..c_hi (mask = label == c) in one call:
 *        border(X)[v] = X[v] and one of the 2*ndim face neighbours is unset or outside the array;
 *        hist[c - c_lo][0][k] = #{v in border(pred == c) : squared distance from v to the nearest voxel of border(gt == c) is k},
 *        hist[c - c_lo][1][k] = the same with pred and gt exchanged;  nbins = (D-1)^2 + (H-1)^2 + (W-1)^2 + 1 bins per row.
 *      Integer arithmetic throughout: the counts do not depend on the order of arrival.  A class without a voxel in either map
 *      gives two rows of zeros.  ndim 2: D must be 1 and the z neighbours do not exist (they are not background).  hist is zeroed
 *      here; ws: arco_surface_ws_bytes(D, H, W, classes) bytes (two uint32 planes per class and direction; -1 for sizes the launch
 *      rejects).  ARCO_ERR_ARG before anything is launched for: a null pointer, a dim < 1 or > 4096, ndim not 2 or 3, ndim 2 with
 *      D != 1, c_hi < c_lo, more than 32 classes, ws_bytes or hist_bytes (classes * 2 * nbins * 8) too small.                    */
long arco_surface_ws_bytes(int D, int H, int W, int nc);
int arco_surface_hist(const int64_t* pred, const int64_t* gt, int D, int H, int W, int ndim, int c_lo, int c_hi, void* ws,
                      long ws_bytes, int64_t* hist, long hist_bytes, void* stream);
/* ---- V  the same surface distances with a voxel spacing (sz, sy, sx > 0 and finite; sz is ignored for ndim 2) and a connectivity
 *      (1..ndim: a neighbour differs by +-1 in 1 to `connectivity` axes, scipy's generate_binary_structure(ndim, connectivity); outside
 *      the array counts as unset), in float64.  With w_a(e) = fl(fl(s_a * e) * fl(s_a * e)) the squared distance of a voxel v to
 *      border(B) is the minimum over the voxels u of border(B) of fl(fl(w_x(dx) + w_y(dy)) + w_z(dz)), (dz, dy, dx) = v - u - every
 *      operation rounded once, none fused, the minimum exact - so an O(n^2) restatement in that order reproduces it bit for bit.
 *      Every voxel of border(A) with a finite squared distance appends one record: val = that float64, tag = (c - c_lo) * 2 + direction
 *      (0: A = pred == c, B = gt == c; 1: exchanged).  The records are packed through an integer cursor (no float atomics); their
 *      order is that of arrival, their multiset is fixed.  count[0] (zeroed here) ends at the true number of records; only the
 *      first min(count, cap) are written - a voxel is in one class per map, so cap = 2 * D * H * W never overflows.
 *      ws: arco_surface_sp_ws_bytes(D, H, W, classes) bytes (two float64 planes per class and direction; -1 for sizes the launch
 *      rejects).  ARCO_ERR_ARG before anything is launched for: a null pointer, a dim < 1 or > 4096, ndim not 2 or 3, ndim 2 with
 *      D != 1, connectivity outside 1..ndim, a spacing that is not finite and > 0, c_hi < c_lo, more than 32 classes, ws_bytes too
 *      small, cap < 1.                                                                                                            */
long arco_surface_sp_ws_bytes(int D, int H, int W, int nc);
int arco_surface_sp_dist(const int64_t* pred, const int64_t* gt, int D, int H, int W, int ndim, int connectivity, double sz, double sy,
                         double sx, int c_lo, int c_hi, void* ws, long ws_bytes, double* val, int32_t* tag, long cap, int64_t* count,
                         void* stream);
/* ---- V  connected components and the largest one (test_util.py:11-15 getLargestCC) of one contiguous integer label volume [D][H][W]:
 *      foreground = x != 0; neighbours differ by +-1 in at most `connectivity` axes (scipy's generate_binary_structure(ndim, connectivity);
 *      1 = faces, ndim = 8 neighbours in 2-D / 26 in 3-D, which is what getLargestCC uses).  ndim 2: D must be 1.
 *        labels[v]  int32: 0 on background, else 1 + the smallest linear index of v's component;
 *        largest[v] uint8: 1 on the component with the most voxels (of several that large: the one whose first voxel comes first);
 *        info       int64[3] = {components, linear index of the winner's first voxel, its voxel count}; {0, -1, 0} without foreground.
 *      Integer arithmetic and order-independent: identical bits on every run.  ws: arco_cc_ws_bytes(D, H, W) bytes, 8-byte aligned (-1
 *      for sizes the launch rejects).  ARCO_ERR_ARG before anything is launched or written for: a null pointer, a dim < 1 or > 4096,
 *      D*H*W >= 2^31, ndim not 2 or 3, ndim 2 with D != 1, connectivity outside 1..ndim, ws_bytes, labels_bytes (4 per voxel),
 *      largest_bytes (1 per voxel) or info_bytes (24) too small.                                                                  */
long arco_cc_ws_bytes(int D, int H, int W);
int arco_cc_largest(const int64_t* x, int D, int H, int W, int ndim, int connectivity, void* ws, long ws_bytes, int32_t* labels,
                    long labels_bytes, uint8_t* largest, long largest_bytes, int64_t* info, long info_bytes, void* stream);
/* ---- V  connected components BY VALUE and the largest one of every class (csrc/cc.hip, arco_amd/utils/cc_gpu.py): what
 *      skimage.measure.label, which the reference's getLargestCC calls, means for more than two classes.  C = classes in 2..256.  A voxel
 *      is in range when 1 <= x[v] <= C - 1; every other value (0, negatives, >= C) is background in all outputs.  Two in-range voxels are
 *      connected when they are neighbours as above AND have equal values.
 *        labels[v]  int32: 0 on background, else 1 + the smallest linear index of v's component;
 *        keep[v]    uint8: 1 where v lies in the component of ITS OWN class with the most voxels (of several that large: the one whose
 *                   first voxel comes first in memory);
 *        info       int64[C + 1][3]: rows 1..C-1 = {components of class c, linear index of the winner's first voxel, its voxel count},
 *                   {0, -1, 0} for an absent class; row 0 the same triple over all classes together (every component; the single one
 *                   with the most voxels, ties to the first in memory); row C = {voxels with a value outside 0..C-1, linear index of
 *                   the first of them or -1, 0}.
 *      Integer arithmetic and order-independent: identical bits on every run.  ws: arco_cc_value_ws_bytes(D, H, W, classes) bytes, 8-byte
 *      aligned (-1 for sizes or a class count the launch rejects).  ARCO_ERR_ARG before anything is launched or written for: a null
 *      pointer, a dim < 1 or > 4096, D*H*W >= 2^31, classes outside 2..256, ndim not 2 or 3, ndim 2 with D != 1, connectivity outside
 *      1..ndim, ws_bytes, labels_bytes (4 per voxel), keep_bytes (1 per voxel) or info_bytes (24 * (C + 1)) too small.              */
long arco_cc_value_ws_bytes(int D, int H, int W, int classes);
int arco_cc_value_largest(const int64_t* x, int D, int H, int W, int ndim, int connectivity, int classes, void* ws, long ws_bytes,
                          int32_t* labels, long labels_bytes, uint8_t* keep, long keep_bytes, int64_t* info, long info_bytes,
                          void* stream);
/* ---- V  the zoom(order=0) round trip of 2-D evaluation (test_2D.py:72-88; csrc/zoom.hip, arco_amd/utils/zoom_gpu.py), bit for bit
 *      scipy.ndimage.zoom(order=0, mode='constant'): output index o of an axis of n_in points resampled to n_out >= 2 points reads input
 *      index floor(cc + 0.5), cc = (double)o * z, z = (n_in - 1) / (n_out - 1) computed by the caller in float64; the output is the
 *      constant 0 where !(0 <= cc <= n_in - 1) (for some sizes the last index lands one ulp above n_in - 1: a whole zeroed last row or
 *      column).  Float64 without contraction; an index depends on o alone, not on the slice.
 *      arco_zoom_nearest2d: src [S][n0][n1] -> out [S][N0][N1], both contiguous, elements of elem_bytes = 4 or 8 bytes moved as bits (fp32
 *      images, int64 label maps); z0 / z1 the steps of the two axes.  Any alignment of `out` is taken (16-byte stores where it allows).
 *      ARCO_ERR_ARG before anything is launched for: a null pointer, S / n0 / n1 < 1, N0 / N1 < 2, elem_bytes not 4 or 8, a z that is
 *      negative or not finite.
 *      arco_argmax_zoom_back2d: the fused tail.  X: logits rows [n * P0 * P1][ld] (channels-last, C <= 32 classes, ld >= C) ->
 *      out int64 [n][N0][N1]: label 0 where the sampled pixel of the P0 x P1 map is outside, else the class arco_softmax_rows returns as
 *      `amax` for that one row (the first strict maximum of the fp32 probabilities, not the arg-max of the logits).  Rows that no output
 *      pixel samples are not read.  ARCO_ERR_ARG before anything is launched for: a null pointer, C < 1 or > 32, ld < C, n / P0 / P1
 *      < 1, N0 / N1 < 2, a z that is negative or not finite.                                                                        */
int arco_zoom_nearest2d(const void* src, int S, int n0, int n1, int N0, int N1, double z0, double z1, int elem_bytes, void* out,
                        void* stream);
int arco_argmax_zoom_back2d(const float* X, long ld, int C, int n, int P0, int P1, int N0, int N1, double z0, double z1, int64_t* out,
                            void* stream);
/*      arco_argmax_zoom_back2d_h: the same on f16 logits rows (the stored logits of the f16 inference route, ops.eval_half(logits="stored")):
 *      every value is widened to fp32 - exact - and goes through the same arithmetic, so `out` is what arco_argmax_zoom_back2d gives for
 *      the fp32 cast of the rows, first maximum on ties included.  8-byte loads where ld % 4 == 0 and X is 8-byte aligned, else one value
 *      at a time.  The same ARCO_ERR_ARG cases.                                                                                     */
int arco_argmax_zoom_back2d_h(const void* X, long ld, int C, int n, int P0, int P1, int N0, int N1, double z0, double z1, int64_t* out,
                              void* stream);
/* ---- V  zoom(order=3) of 2-D evaluation (the reference's test.py:124; csrc/zoom.hip, arco_amd/utils/zoom_gpu.py):
 *      scipy.ndimage.zoom(a, f, order=3) with scipy's defaults (mode='constant', cval=0, prefilter=True, grid_mode=False) of float32
 *      slices, as two steps in float64 without contraction, every operation in the order tests/zoom_cubic_kernel_refs.py restates.
 *      arco_spline_prefilter2d: src float32 [S][n0][n1] -> out float64 B-spline coefficients [S][n0][n1].  Along every line of n points,
 *      axis 0 (axes & 1) then axis 1 (axes & 2; alone it filters `out` in place and reads no `src`): the gain, the causal initial sum
 *      over the whole line (mirror boundary), the causal and the anticausal recursion, strictly in sequence.  z = sqrt(3) - 2,
 *      gain = (1 - z)(1 - 1 / z), zn0 = z^(n0 - 1), zn1 = z^(n1 - 1) are computed by the caller in float64.  ARCO_ERR_ARG before
 *      anything is launched for: a null pointer, S < 1, n0 / n1 < 2, axes outside 1..3, a z / gain / zn that is not finite.
 *      arco_zoom_cubic2d: coef [S][n0][n1] -> out float32 [S][N0][N1].  Output index o of an axis samples cc = (double)o * z,
 *      z = (n_in - 1) / (n_out - 1) from the caller; the output is 0 where !(0 <= cc <= n_in - 1), else the sum over the 4 x 4 taps
 *      floor(cc) - 1 .. + 2 (mirrored into [0, n_in - 1]) of coef * w_axis0 * w_axis1, cast to float32.  Any alignment of `out`.
 *      ARCO_ERR_ARG before anything is launched for: a null pointer, S < 1, n0 / n1 < 2 or > 2^30, N0 / N1 < 2, a z that is negative
 *      or not finite.                                                                                                              */
int arco_spline_prefilter2d(const float* src, int S, int n0, int n1, double z, double gain, double zn0, double zn1, int axes, double* out,
                            void* stream);
int arco_zoom_cubic2d(const double* coef, int S, int n0, int n1, int N0, int N1, double z0, double z1, float* out, void* stream);
/* ---- A  mixing strategies of the unlabeled stream (augment.py:284-313 generate_unsup_data, masks :230-252; volumes
 *      augment_3d.py:182-257).  desc_host[B][8] = {y0, y1, x0, x1, z0, z1, sel_lo, sel_hi} in HOST memory (the host
 *      draws it; it travels in the kernel arguments); Z = 1 in 2-D; mode 0 cutmix, 1 cutout, 2 classmix; data NC[spatial] */
int arco_mix_unsup(const float* data, int Cimg, const int64_t* target, const float* logits, int B, int H, int W, int Z,
                   const int* desc_host, int mode, float* odata, int64_t* otarget, float* ologits, void* stream);
/*      presence[i] = bit set of the labels occurring in target[i] (torch.unique of augment.py:248), labels < 64          */
int arco_label_presence(const int64_t* target, int B, long HW, uint64_t* presence, void* stream);
/* ---- V  3-D sliding-window evaluation (test_util.py:139-211): score[C][ww][hh][dd] += prob[C][px][py][pz] at (xs, ys, zs),
 *      cnt += 1 (test_util.py:196-199); then score /= cnt, label = argmax over classes (:200-201)                    */
int arco_window_accumulate(const float* prob, int C, int px, int py, int pz, float* score, float* cnt, int ww, int hh, int dd,
                           int xs, int ys, int zs, void* stream);
int arco_score_finalize(float* score, const float* cnt, int C, long vol, int64_t* label, void* stream);
long arco_seg_ws_doubles(long M, int C, int B);
int arco_sup_loss_fwd(const float* X, long ld, long M, int C, const int64_t* lab, double* ws, float* out, void* stream);
int arco_sup_loss_bwd(const float* X, long ld, long M, int C, const int64_t* lab, const double* ws, const float* g_ce,
                      const float* g_dice, float* dX, long ldo, void* stream);
/* utils/losses.py:173-209 DiceLoss.forward on probability rows [M, C] (what train_arco_2d.py:269,338 /
 * train_arco_3d.py:245,308 instantiate and call): per-class weights or NULL; ws as for arco_sup_loss_fwd                  */
int arco_dice_probs_fwd(const float* P, long ld, long M, int C, const int64_t* lab, const float* wgt, double* ws, float* out,
                        void* stream);
int arco_dice_probs_bwd(const float* P, long ld, long M, int C, const int64_t* lab, const float* wgt, const double* ws,
                        const float* g, float* dP, long ldo, void* stream);
/* workspaces of the two per-image losses: unsup ws >= arco_loss_slabs(B) * 4 * B + B + 1 doubles, eqv ws >= arco_loss_slabs(B) * 2 * B + B */
long arco_loss_slabs(int B);
int arco_unsup_loss_fwd(const float* X, long ld, int B, long P, int C, const int64_t* lab, const float* conf, float thr,
                        double* ws, float* out, void* stream);
int arco_unsup_loss_bwd(const float* X, long ld, int B, long P, int C, const int64_t* lab, const double* ws, const float* g,
                        float* dX, long ldo, void* stream);
long arco_sel_state_bytes();
/* exact np.percentile(entropy[valid], q) (linear) by device radix select -> low/high masks              */
int arco_entropy_masks(const float* ent, const int64_t* lab_l, const int64_t* lab_u, long n_l, long n_u, double q_lo,
                       double q_hi, void* state, float* low, float* high, void* stream);
/*      the same in phases for data-parallel runs: all-reduce the field at arco_sel_state_offset(0) (uint64 valid count)
 *      after phase 0 and the field at arco_sel_state_offset(1) (uint32 hist[4][256]) after every phase 2; phases:
 *      0 clear + count, 1 ranks, 2 histogram of digit `pass`, 3 pick digit `pass`, 4 masks                              */
long arco_sel_state_offset(int field);
int arco_entropy_masks_phase(int phase, int pass, const float* ent, const int64_t* lab_l, const int64_t* lab_u, long n_l,
                             long n_u, double q_lo, double q_hi, void* state, float* low, float* high, void* stream);

/* ---- L4  HOST entry points (CPU memory, no stream): native replay of the stratified samplers
 *      grid_monte_carlo_sample / grid_as_monte_carlo_sample (loss_helper_3d.py:120-268) on the
 *      serialized torch CPU generator state (torch.get_rng_state()), bit-exact incl. final state.        */
long arco_grid_sample(uint8_t* state, long state_bytes, long high, long shape, int cut, int mirror, int64_t* out);
/* a sequence of sampler calls in generator order; value-independent calls run on state copies in worker threads
 * while the generator is skipped ahead.  Returns the index of the first call that needs the 1-D fallback
 * (n_jobs when all ran; `state` = generator state right before that call), <0 on error.                       */
long arco_grid_sample_many(uint8_t* state, long state_bytes, int n_jobs, const long* highs, const long* shapes, int cut,
                           int mirror, int64_t* const* outs, int max_threads);
/* deferred form: returns once the generator's final state is known (inline calls done, worker calls launched - their
   draw counts are fixed); arco_grid_sample_many_finish() waits for the worker calls' outputs.  The trainer draws the
   equivariance warp (train_arco_2d.py:412, the next consumer of the CPU generator) and queues that pass in between.  */
long arco_grid_sample_many_async(uint8_t* state, long state_bytes, int n_jobs, const long* highs, const long* shapes, int cut,
                                 int mirror, int64_t* const* outs, int max_threads);
void arco_grid_sample_many_finish(void);
long arco_randint(uint8_t* state, long state_bytes, long high, long n, int64_t* out);
/* generator consumption of a draw whose values are not needed: advance the serialized torch CPU generator by n 32-bit
 * draws (train_arco_2d.py:156 `torch.randn(K, 496, H, W)` when the revisiting term is off)                              */
long arco_mt_skip(uint8_t* state, long state_bytes, uint64_t n);
/* the generator's next state blocks for >= n_draws draws, computed ahead of time from `state` (not modified; in a worker
   thread when background != 0) while the host waits for the GPU's per-class counters (loss_helper_3d.py:413-434 needs them
   before the first sampler call :435-476).  The next arco_grid_sample_many call that starts from exactly this state reads
   the blocks instead of regenerating (skip-ahead O(1): the big calls run in parallel, the 16 grid blocks of an anchor call
   too); from any other state they are ignored.  Same draws, same final generator state.                              */
long arco_mt_pregen(const uint8_t* state, long state_bytes, long n_draws, int background);

/* ---- f16 ACTIVATION STORAGE of the volume path (BASELINE.json configs[4] "fp16 MFMA conv"; csrc/conv_h.hip) --------------
 * The V-Net body (vnetWithArgs.py:5-31 ConvBlock, :67-91 DownsamplingConvBlock, :94-118 UpsamplingDeconvBlock, :145-252 VNet)
 * with every activation and activation gradient held as f16 in HBM; weights, BatchNorm statistics, parameter gradients,
 * loss and optimizer fp32.  Entry points that take f16 tensors:
 *   arco_conv3d_fwd(..., mma = 4):   `in` and `out` are f16 rows (taps 27 with K = 1: `in` is the fp32 one-channel volume, `out`
 *                                    f16), Wp is the f16 pack of arco_pack_conv_weight(mode | 4) = [taps][ceil16(N)][ceil32(K)]
 *                                    halves (the K = 1 layer: the fp32 pack); v_mfma_f32_16x16x32_f16, fp32 accumulate, BN partials
 *                                    of the rounded outputs; no residual operand.
 *   arco_conv3d_wgrad(..., mma = 4): dZ and `in` f16 (Cin = 1: `in` fp32), dW fp32; operands transposed by ds_read_b64_tr_b16.
 *   arco_chan_stats_h / arco_bn_act_fwd_h / arco_bn_act_bwd_h / arco_colsum_h: the fp32 entry points of the same name on f16
 *                                    tensors (fp32 arithmetic, statistics and parameter gradients).
 *   arco_cast_h2f / arco_cast_f2h:   the region's boundary: outputs to fp32; fp32 gradients in, multiplied by the loss scale.
 * Space-to-depth (arco_s2d3) is a permutation of 4-byte words: f16 tensors pass with C / 2 and ld / 2.                       */
int arco_chan_stats_h(const void* X, long ldx, long M, int C, float* ssum, float* ssq, int groups, void* stream);
int arco_bn_act_fwd_h(const void* Z, long ldz, long M, int C, const float* mean, const float* istd, const float* gamma,
                      const float* beta, float slope, int drop_mode, float p, uint64_t seed, long P, void* A, long lda,
                      const uint64_t* seed_dev, int groups, void* stream);
int arco_bn_act_bwd_h(const void* dA, long ldd, const void* Z, long ldz, long M, int C, const float* mean,
                      const float* istd, const float* gamma, const float* beta, float slope, int drop_mode, float p,
                      uint64_t seed, long P, float* ws, float* dgamma, float* dbeta, int accumulate, void* dZ, long ldo,
                      const uint64_t* seed_dev, int groups, void* stream);
int arco_colsum_h(const void* X, long ldx, long M, int C, float* ws, float* out, int accumulate, void* stream);
/* A = lrelu(BN(Z)) + R: the apply pass of UpsamplingDeconvBlock's BatchNorm with the decoder's skip addition folded in
 * (vnetWithArgs.py:224-236 `x5_up = self.block_five_up(x5) + x4` ...); mean / istd rows [groups][C] as for arco_bn_act_fwd      */
int arco_bn_act_add_fwd(const float* Z, long ldz, long M, int C, const float* mean, const float* istd, const float* gamma,
                        const float* beta, float slope, const float* R, long ldr, float* A, long lda, int groups, void* stream);
int arco_bn_act_add_fwd_h(const void* Z, long ldz, long M, int C, const float* mean, const float* istd, const float* gamma,
                          const float* beta, float slope, const void* R, long ldr, void* A, long lda, int groups, void* stream);
/* UpsamplingDeconvBlock's BatchNorm + ReLU (+ skip) straight from the GEMM form of the k2 s2 transposed conv (vnetWithArgs.py:94-118):
 * Y = [voxels of the NV x X2 x Y2 x Z2 grid][8 C] (tap-major channels, tap = dx*4 + dy*2 + dz) is read as M8 = 8 * voxels rows of C
 * channels - the pre-activation in (voxel, tap) row order; statistics: arco_chan_stats(Y, ld = C, M8, C); the apply pass writes row
 * (voxel, tap) to voxel (n, 2x+dx, 2y+dy, 2z+dz) of A (and adds R there), the backward reads dA from there and leaves dY in Y's
 * order - no depth-to-space / space-to-depth pass in either direction.                                                            */
int arco_bn_act_d2s_fwd(const float* Y, long M8, int C, const float* mean, const float* istd, const float* gamma, const float* beta,
                        float slope, const float* R, long ldr, float* A, long lda, int X2, int Y2, int Z2, int groups, void* stream);
int arco_bn_act_d2s_fwd_h(const void* Y, long M8, int C, const float* mean, const float* istd, const float* gamma, const float* beta,
                          float slope, const void* R, long ldr, void* A, long lda, int X2, int Y2, int Z2, int groups, void* stream);
int arco_bn_act_d2s_bwd(const float* dA, long ldd, const float* Y, long M8, int C, const float* mean, const float* istd,
                        const float* gamma, const float* beta, float slope, float* ws, float* dgamma, float* dbeta, int accumulate,
                        float* dY, int X2, int Y2, int Z2, int groups, void* stream);
int arco_bn_act_d2s_bwd_h(const void* dA, long ldd, const void* Y, long M8, int C, const float* mean, const float* istd,
                          const float* gamma, const float* beta, float slope, float* ws, float* dgamma, float* dbeta, int accumulate,
                          void* dY, int X2, int Y2, int Z2, int groups, void* stream);
/* V = depth_to_space(P) + ADD: the gradient of an encoder activation that feeds both the next DownsamplingConvBlock (through
 * space-to-depth) and the decoder's skip connection (vnetWithArgs.py:186-201,224-236), one pass instead of arco_s2d3 + an add    */
/* (non-null pointers, 16-byte aligned - f16: 8-byte -, positive sizes, C and the strides multiples of 4) */
int arco_d2s3_add(const float* P, long ldp, int NV, int X2, int Y2, int Z2, int C, const float* ADD, long lda, float* V, long ldv, void* stream);
int arco_d2s3_add_h(const void* P, long ldp, int NV, int X2, int Y2, int Z2, int C, const void* ADD, long lda, void* V, long ldv, void* stream);
int arco_cast_h2f(const void* x, long n, float* y, void* stream);
int arco_cast_f2h(const float* x, long n, float scale, void* y, void* stream);
/* f16 activation storage on the 2-D path (train_arco_2d --act_dtype f16; the _Float16 instantiations of csrc/elementwise.hip).  The 3x3 convolutions of f16 maps run
 * through arco_conv3d_fwd / arco_conv3d_wgrad(taps = 9, D3 = 1, mma = 4): hconv_kernel's plane step without the depth loop, rows
 * that are not whole 16-byte pieces (the gradient of a 4- / 19-class out_conv) staged element-wise.
 *   arco_conv3x3_image_fwd_h:    the first layer - fp32 image (K <= 4 channels, the fp32 forward pack [9][16][16]) -> f16 map of
 *                                N <= 16 channels + BatchNorm partials of the rounded values, one slab per workgroup
 *                                (arco_conv3x3_image_mblocks_h of them).
 *   arco_conv3x3_image_wgrad_h:  its weight gradient from the f16 dZ (16 channels) and the fp32 image; ws as arco_wgrad_ws_floats.
 *   arco_maxpool2_*_h / arco_bilinear_*_h: the fp32 entry points of the same name on f16 tensors (C % 8 == 0, rows of whole
 *                                16-byte pieces): fp32 arithmetic, one rounding on store.
 *   arco_bn_act_pool_fwd_h:      arco_bn_act_pool_fwd on f16 tensors (the f16 inference route of the U-Net's encoder blocks): Z is
 *                                read once, A = lrelu(BN(Z)) is formed in fp32 by arco_bn_act_fwd_h's expression and rounded once,
 *                                P = the 2x2 maximum of the rounded values - both outputs bit for bit arco_bn_act_fwd_h followed by
 *                                arco_maxpool2_fwd_h.  lda may exceed C (concat room: the other channels are not touched).  C and
 *                                the strides multiples of 4, H and W even, the f16 pointers 8-byte and the parameter pointers
 *                                16-byte aligned; 16-byte lanes where C % 8 == 0 and every row is whole 16-byte pieces.        */
int arco_conv3x3_image_mblocks_h(int NB, int H, int W, int stat_groups);
int arco_conv3x3_image_fwd_h(const float* in, long ld_in, int K, const float* Wp, int N, void* out, long ld_out, const float* bias,
                             float* stat_sum, float* stat_sq, int NB, int H, int W, int stat_groups, void* stream);
int arco_conv3x3_image_wgrad_h(const void* dZ, long ld_dz, int Cout, const float* in, long ld_in, int K, int NB, int H, int W,
                               float* ws, float* dW, int accumulate, void* stream);
int arco_maxpool2_fwd_h(const void* X, long ldx, int NB, int H, int W, int C, void* Y, long ldy, void* stream);
int arco_bn_act_pool_fwd_h(const void* Z, long ldz, int NB, int H, int W, int C, const float* mean, const float* istd,
                           const float* gamma, const float* beta, float slope, void* A, long lda, void* P, long ldp, int groups,
                           void* stream);
int arco_maxpool2_bwd_h(const void* X, long ldx, int NB, int H, int W, int C, const void* dY, long ldy, void* dX, long ldo,
                        void* stream);
int arco_maxpool2_bwd_add_h(const void* X, long ldx, int NB, int H, int W, int C, const void* dY, long ldy, const void* add,
                            long ld_add, void* dX, long ldo, void* stream);
int arco_bilinear_fwd_h(const void* X, long ldx, int NB, int Hi, int Wi, int C, int Ho, int Wo, void* Y, long ldy, void* stream);
int arco_bilinear_bwd_h(const void* dY, long ldy, int NB, int Hi, int Wi, int C, int Ho, int Wo, void* dX, long ldx, void* stream);
/* Data ingest from a GPU-resident dataset (trainers' --gpu_ingest 1; csrc/ingest.hip, arco_amd/dataloaders/gpu_ingest.py): one launch
 * per batch reproduces the host transforms bit for bit - 2-D: zoom(order=0) to the patch, then none / rot90 + flip / rotate(order=0) /
 * centre crop; 3-D: RandomRotFlip -> RandomCrop -> ToTensor.  bank_img / bank_lab: the packed cases (fp32 / uint8, bank_elems elements
 * each); table: [n_cases][4] int64 {offset, n0, n1, n2}; desc, on the device: 2-D [B][16] float64 {case, op, Z0, Z1, z0, z1, a, b, m00, m01,
 * m10, m11, off0, off1, -, -}, 3-D [B][8] int64 {case, k, axis, s0, s1, s2, -, -}.  out_img [B,1,...] fp32, out_lab [B,...] int64 or null;
 * the fastest output axis a multiple of 4.  Coordinates in float64 without contraction (scipy.ndimage's order-0 rule). */
int arco_ingest_slices(const float* bank_img, const unsigned char* bank_lab, long bank_elems, const long* table, long n_cases,
                       const double* desc, int B, int H, int W, float* out_img, long* out_lab, void* stream);
int arco_ingest_volumes(const float* bank_img, const unsigned char* bank_lab, long bank_elems, const long* table, long n_cases,
                        const long* desc, int B, int X, int Y, int Z, float* out_img, long* out_lab, void* stream);
/* The student transform of stage-1 pre-training (pretrain_2D / pretrain_3D --gpu_ingest 1; csrc/stage1_aug.hip,
 * arco_amd/dataloaders/stage1_aug.py) on PLANES of one fp32 buffer of n_elems elements: plane p = (j, t) = (p / T, p % T) starts at element
 * j * s_img + t * s_t, pixel (r, c) is r * s_row + c * s_col further on (2-D [B,1,H,W]: T = 1, s_row = W, s_col = 1; 3-D [B,1,X,Y,Z],
 * planes [j,0,:,:,t]: T = Z, s_t = 1, s_row = Y * Z, s_col = Z).  Planes p >= n_planes are not touched.
 * arco_gray_jitter_planes: torchvision's tensor-mode ColorJitter on one-channel planes, in place; recs = n_planes records
 *   {int order[4]; float fb, fc;} (arco_jit_record_bytes) in DEVICE memory; op 0: x = clamp(x * fb, 0, 1), op 1: x = clamp(x * fc +
 *   (1 - fc) * mean, 0, 1) with the plane's mean summed in float64 in a fixed order (no atomics), ops 2 / 3 nothing; no contraction.
 * arco_blur_planes: Pillow's GaussianBlur of trunc(clamp(x * 255)) with ONE fractional box radius in [0, 1) for all planes (anything
 *   else: ARCO_ERR_UNSUPPORTED).  out != null: out [n_planes,H,W] fp32 = byte / 255, apart from data.  out == null: in place,
 *   data = (float)byte, blurred into the scratch ws (arco_blur_planes_ws_bytes) and stored back by a second launch. */
long arco_jit_record_bytes(void);
int arco_gray_jitter_planes(float* data, long n_elems, long n_planes, int T, int H, int W, long s_img, long s_t, long s_row, long s_col,
                            const void* recs, void* stream);
long arco_blur_planes_ws_bytes(long n_planes, int T, int H, int W);
int arco_blur_planes(float* data, long n_elems, long n_planes, int T, int H, int W, long s_img, long s_t, long s_row, long s_col, float radius,
                     float* out, void* ws, void* stream);

/* The patch-wise pooling of the stage-1 output heads (pretrain_2D / pretrain_3D --patch_heads gpu; csrc/patch_pool.hip, arco_amd/stage1.py).
 * nd = 2: x [B,C,n0,n1] (n2 ignored), nd = 3: x [B,C,n0,n1,n2], fp32 contiguous.  On every spatial axis the patches start at 0, step,
 * 2 * step, ... while start + patch <= n, step = patch / 2; patch number p counts the first spatial axis outermost.  Cell i of a patch
 * covers the local coordinates [floor(i * patch / pool), ceil((i + 1) * patch / pool)) (adaptive average pooling; pool need not divide
 * patch and may exceed it).
 * fwd: y [P,B,C,pool,pool(,pool)] = the window's fp32 sum (axis 0 outermost, ascending) divided once by its element count.
 * bwd: gx [B,C,n...] = per voxel the fp32 sum of gy / count(cell) over the (patch, cell) tuples whose window holds it, nested loops
 *   p0, i0, p1, i1, p2, i2 from the outermost, all ascending; 0 where no patch covers the voxel; every element of gx is written.
 * No atomics: two runs give the same bits.  ARCO_ERR_ARG before any launch for nd outside {2, 3}, patch < 2, pool < 1, B or C < 1, an
 * axis shorter than patch, or a null pointer. */
int arco_patch_pool_fwd(const float* x, int nd, int B, int C, int n0, int n1, int n2, int patch, int pool, float* y, void* stream);
int arco_patch_pool_bwd(const float* gy, int nd, int B, int C, int n0, int n1, int n2, int patch, int pool, float* gx, void* stream);

/* The patch-wise output heads as one kernel each way (pretrain_2D / pretrain_3D --patch_heads fused; csrc/patch_head.hip, arco_amd/stage1.py
 * PatchHeadFn): the pooling above followed by `layers` (1 .. 4) pointwise layers without a non-linearity between them.  Geometry arguments as
 * above.  Widths C = c_0, c_1 .. c_L, every one 1 .. 32; c_k of a layer behind `layers` is ignored.  w_k [c_k, c_{k-1}] fp32 row-major (a
 * kernel-1 convolution weight), non-null for k <= layers and null behind; b_k [c_k] or null: no bias.  A POSITION is one (patch, batch,
 * cell) triple, P * B * pool^nd of them.
 * fwd: pooled [P,B,C,pool...] = arco_patch_pool_fwd's values, bit for bit; y [P*B,c_L,pool...]; per position, in fp32, every operation
 *   rounded on its own: a_k[j] = b_k[j] (0.f without bias), then a_k[j] = a_k[j] + w_k[j,i] * a_{k-1}[i] for i ascending; y = a_L.
 * bwd: gy in the layout of y.  Per position a_0 .. a_{L-1} again from pooled, d_L = gy, d_{k-1}[i] = 0.f, then d_{k-1}[i] = d_{k-1}[i] +
 *   w_k[j,i] * d_k[j] for j ascending.  d0 [P,B,C,pool...] = d_0, or null: not wanted (arco_patch_pool_bwd takes it to the input).
 *   The parameter gradients dw_k[j,i] = sum of (double)d_k[j] * (double)a_{k-1}[i], db_k[j] = sum of (double)d_k[j] over the positions
 *   are accumulated in float64 into ws (arco_patch_head_ws_bytes; one slab per workgroup), without atomics and in an order that depends
 *   on the position count and the widths alone: two runs give the same bits.
 * wgrad_finish: the slabs of ws added in ascending order in float64, rounded once into gw_k [c_k, c_{k-1}] / gb_k [c_k] fp32; a null
 *   pointer: that gradient is not wanted.  Same geometry, layers and widths as the bwd call that filled ws.
 * ARCO_ERR_ARG before any launch for the pooling's refusals, layers outside 1 .. 4, a width above 32 or below 1, a null w_k of a present
 * layer, a non-null pointer of an absent one, or a null tensor.  arco_patch_head_ws_bytes returns -1 for such arguments. */
long arco_patch_head_ws_bytes(int nd, int B, int C, int n0, int n1, int n2, int patch, int pool, int layers, int c1, int c2, int c3, int c4);
int arco_patch_head_fwd(const float* x, int nd, int B, int C, int n0, int n1, int n2, int patch, int pool, int layers,
                        const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                        const float* w4, const float* b4, int c1, int c2, int c3, int c4, float* pooled, float* y, void* stream);
int arco_patch_head_bwd(const float* pooled, const float* gy, int nd, int B, int C, int n0, int n1, int n2, int patch, int pool, int layers,
                        const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                        const float* w4, const float* b4, int c1, int c2, int c3, int c4, float* d0, double* ws, void* stream);
int arco_patch_head_wgrad_finish(const double* ws, int nd, int B, int C, int n0, int n1, int n2, int patch, int pool, int layers,
                                 int c1, int c2, int c3, int c4, float* gw1, float* gb1, float* gw2, float* gb2, float* gw3, float* gb3,
                                 float* gw4, float* gb4, void* stream);

/* The KL-divergence-to-queue loss of stage 1 as two kernels (pretrain_2D / pretrain_3D --kld fused; csrc/queue_kld.hip, arco_amd/stage1.py
 * QueueKLDFn): loss = F.kl_div(F.log_softmax(cs / Ts, 1), F.softmax(ct / Tt, 1), 'batchmean') of two row-major fp32 matrices of raw cosines
 * cs, ct [N, L] with row strides ld_s, ld_t >= L (in floats) and the inverse temperatures inv_ts = 1 / Ts, inv_tt = 1 / Tt, both > 0 and finite.
 * fwd: one pass over each matrix (online softmax with the true running row maxima).  stats [N, 3] float64 = per row lse_s, lse_t and
 *   KL_i = sum_j p_ij ((t_ij - lse_t) - (s_ij - lse_s)), s = cs * inv_ts, t = ct * inv_tt, p = softmax(t); a term with p_ij = 0 adds 0.
 *   loss [1] fp32 = (sum of KL_i in float64, in a fixed order) / N, from a second small launch.  A non-finite cosine makes the loss non-finite.
 * bwd: g [1] fp32 on the device, the gradient of the loss.  dcs_ij = g (softmax(s)_ij - p_ij) inv_ts / N with row stride ld_ds,
 *   dct_ij = g p_ij ((t_ij - lse_t) - (s_ij - lse_s) - KL_i) inv_tt / N with row stride ld_dt; a null dcs or dct: not wanted (not both).
 *   dcs may be cs and dct may be ct (then with that matrix's stride): the gradient replaces the cosines.  Any other overlap of the four
 *   matrices is the caller's error; dcs == ct, dct == cs and dcs == dct are refused.
 * Rows of up to arco_queue_kld_short_max() elements take one wave each, longer rows one workgroup of 256 threads each; 16-byte accesses
 * where L, every stride and every pointer allow them, scalar ones otherwise.  No atomics: two runs give the same bits.
 * ARCO_ERR_ARG before any launch for a null pointer, N or L outside 1 .. 2^31 - 1, a stride below L or above 2^31 - 1, or a temperature
 * factor that is not positive and finite. */
long arco_queue_kld_short_max(void);
int arco_queue_kld_fwd(const float* cs, const float* ct, long N, long L, long ld_s, long ld_t, float inv_ts, float inv_tt, double* stats,
                       float* loss, void* stream);
int arco_queue_kld_bwd(const float* cs, const float* ct, long N, long L, long ld_s, long ld_t, float inv_ts, float inv_tt, const double* stats,
                       const float* g, float* dcs, long ld_ds, float* dct, long ld_dt, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARCO_HIP_H */
