/* tamtr_hip.h - C ABI of libtamtr_hip.so: hand-written CDNA4 (gfx950 / MI355X) kernels for the TAM-TR
 * text-image attention hot path (BTA-PAN max-sigmoid text gate + MEH deformable-attention decoder).
 *
 * The reference (Xjh-UCAS/TAM-TR) is 100 % Python and has no FFI of its own; each entry point
 * below therefore cites the reference *Python* interface whose arithmetic it replaces (paths relative to the
 * reference root).  INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM), row-major/contiguous in the layout stated per function;
 *   - `dtype`: element type of the activation tensors marked (T): TAMTR_F32 or TAMTR_BF16.  Index/offset/weight
 *     side inputs and all accumulation are always fp32;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Functions only enqueue work: no
 *     allocation, no synchronisation, no mutable globals (three A/B switches, TAMTR_GEMM, TAMTR_SELFATTN_SCALAR and TAMTR_SCAN_FWD4, are read from the
 *     environment ONCE, into constants; the LDS-size attribute of the kernels that need > 64 KB is set on every call, i.e. for whichever
 *     device is current) - they are safe to call from several host threads on different streams and devices and can be captured into a
 *     hipGraph;
 *   - return value: 0 = enqueued; TAMTR_EINVAL (bad argument), TAMTR_EUNSUP (shape/dtype outside what the kernels
 *     are built for), TAMTR_ELAUNCH (HIP reported a launch error).  Nothing is ever thrown across the ABI.
 */
#ifndef TAMTR_HIP_H
#define TAMTR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAMTR_F32 0
#define TAMTR_BF16 1

#define TAMTR_OK 0
#define TAMTR_EINVAL (-1)
#define TAMTR_EUNSUP (-2)
#define TAMTR_ELAUNCH (-3)

/* ABI version, bumped on any signature change.  The CLIP text tower's entries at the end of this file (tamtr_text_embed, tamtr_linear_f32,
 * tamtr_text_pool_project), tamtr_val_confusion, tamtr_val_ap_curves / tamtr_val_ap_tile and tamtr_bytetrack_update / tamtr_botsort_update /
 * tamtr_bytetrack_workspace_bytes, tamtr_val_coco_match / tamtr_val_coco_workspace_bytes / tamtr_val_coco_accumulate and tamtr_mot_update /
 * tamtr_mot_end_sequence / tamtr_mot_workspace_bytes, tamtr_hota_update / tamtr_hota_end_sequence / tamtr_hota_workspace_bytes,
 * tamtr_trackmap_update / tamtr_trackmap_end_sequence / tamtr_trackmap_workspace_bytes, tamtr_dw_slices / tamtr_dw_bf16 and the stream forms
 * tamtr_bytetrack_update_streams / tamtr_botsort_update_streams / tamtr_botsort_reid_update_streams / tamtr_gmc_estimate_streams and
 * tamtr_mot_update_streams / tamtr_mot_end_streams / tamtr_hota_update_streams / tamtr_hota_end_streams with their workspace sizes are new
 * symbols only: no existing signature changed, so the version stayed at 36 when they were added. */
int tamtr_abi_version(void);

/* ---------------------------------------------------------------------------------------------------------------
 * a-1  Max-sigmoid text gate.   Replaces the body of MaxSigmoidAttnBlock.forward,
 *      ultralytics/nn/extra_modules/block.py:217-226 (dup ultralytics/nn/modules/block.py:672-681):
 *          aw  = sigmoid( max_n( <x[b,m,:,p], gk[b,n,m,:]> ) / sqrt(hc) + bias[m] ) * scale
 *          out = v * aw           (broadcast over the hc channels of head m)
 *      x   (T) [B, nh*hc, HW]   NCHW feature map (embed == x: `ec` is None in every TAM-TR instance)
 *      gk  f32 [B, T, nh*hc]    guide after the `gl` Linear (block.py:212-213)
 *      bias f32 [nh]            scale: python float (1.0 in TAM-TR)
 *      v   (T) [B, nh*hc, HW]   proj_conv(x) (Conv3x3+BN, block.py:223)
 *      out (T) [B, nh*hc, HW]
 *      aw  f32 [B, nh, HW]      saved gate (post-sigmoid, pre-scale)      } consumed by _bwd
 *      arg i32 [B, nh, HW]      argmax text index per pixel and head      }
 */
int tamtr_maxsigmoid_gate_fwd(const void* x, const float* gk, const float* bias, const void* v, void* out, float* aw,
                              int32_t* arg, int B, int nh, int hc, int HW, int T, float scale, int dtype, void* stream);

/*      Backward of the above.  dout (T) [B,C,HW] ->
 *      dx (T) [B,C,HW]    gradient through the embed operand (add to the conv's input gradient on the host side)
 *      dv (T) [B,C,HW]    gradient of proj_conv's output
 *      dlogit f32 [B,nh,HW]  d loss / d (max_n <x,gk>)  (host reduces it into dgk / dbias with one small batched GEMM)
 */
int tamtr_maxsigmoid_gate_bwd(const void* dout, const void* x, const float* gk, const void* v, const float* aw,
                              const int32_t* arg, void* dx, void* dv, float* dlogit, int B, int nh, int hc, int HW, int T,
                              float scale, int dtype, void* stream);
/*      Channels-last forward with the branches' BatchNorm folded into the load (`self.proj_conv` = Conv3x3 + BN,
 *      block.py:205,223; `self.ec`, block.py:203): e (T) [B*HW, C] with row pitch ld_e elements (embed; a channel slice of a wider
 *      NHWC map is fine), v (T) [B*HW, C] packed = the RAW convolution output of the value branch; mean_rstd_* f32 [C][2] (batch mean,
 *      1/sqrt(var + eps), as tamtr_bncl_stats writes them), gamma_* / beta_* f32 [C]; a NULL mean_rstd_* means "already normalised /
 *      no BatchNorm" for that operand.  out (T) [B*HW, C] packed; aw / arg as above or NULL when no backward will follow.
 *      C = nh*hc <= 512, C/8 and hc/8 powers of two; e, v, out, gk 16-byte aligned, ld_e % 8 == 0 (bf16) / % 4 == 0 (f32): a lane
 *      moves the 8 channels it owns as 16-byte pieces, four pixel rows of them in flight (round 4).
 */
int tamtr_maxsigmoid_gate_cl_fwd(const void* e, long long ld_e, const float* mean_rstd_e, const float* gamma_e, const float* beta_e,
                                 const void* v, const float* mean_rstd_v, const float* gamma_v, const float* beta_v, const float* gk,
                                 const float* bias, void* out, float* aw, int32_t* arg, int B, int nh, int hc, int HW, int T, float scale,
                                 int dtype, void* stream);

/*      next-3: the value branch itself.  Replaces `self.proj_conv(x)` = Conv(c1, c2, k=3, s=1, act=False) = nn.Conv2d(3x3, stride 1,
 *      pad 1, no bias) + nn.BatchNorm2d in training mode (ultralytics/nn/extra_modules/block.py:205,223; Conv: nn/modules/conv.py)
 *      for channels-last bf16 maps: an implicit-GEMM MFMA convolution whose epilogue leaves the BatchNorm's batch statistics, to be
 *      followed by tamtr_maxsigmoid_gate_cl_fwd, which applies the affine in its load.  Forward only (TIAGELAN discards the gate: SURVEY D2).
 *      x   bf16 [B*H*W, C1] with row pitch ld_x elements (a channel slice of a wider NHWC map is fine; 16-byte aligned, ld_x % 8 == 0)
 *      wpk bf16 [C1/32][9][C2][32]   the weight [C2][C1][3][3] repacked by tamtr_conv3x3_pack_weight (w: TAMTR_F32 or TAMTR_BF16)
 *      y   bf16 [B*H*W, C2] packed   the RAW convolution output (fp32 accumulation, rounded once)
 *      partials f32 [C2][S][3], S = tamtr_conv3x3_tiles(B, H, W): (count, mean, M2) of the stored values per pixel tile
 *      mean_rstd f32 [C2][2] (batch mean, 1/sqrt(biased var + eps)); running_mean / running_var f32 [C2] or both NULL: updated with
 *      `momentum` (unbiased variance), as nn.BatchNorm2d does.  mean_rstd NULL: convolution + partials only.
 *      C1 % 32 == 0, C2 % 64 == 0.  tamtr_bn_finalize: the per-channel combine on its own (partials [C][S][3] -> mean_rstd, running update).
 */
int tamtr_conv3x3_tiles(int B, int H, int W);
int tamtr_conv3x3_pack_weight(const void* w, void* wpk, int C1, int C2, int dtype, void* stream);
int tamtr_conv3x3_cl_stats_fwd(const void* x, long long ld_x, const void* wpk, void* y, float* running_mean, float* running_var,
                               float* mean_rstd, float* partials, int B, int H, int W, int C1, int C2, float eps, float momentum,
                               void* stream);
int tamtr_bn_finalize(const float* partials, float* mean_rstd, float* running_mean, float* running_var, int C, int S, float eps,
                      float momentum, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * a-6  Multi-scale deformable attention core.  Replaces multi_scale_deformable_attn_pytorch,
 *      ultralytics/nn/modules/utils.py:42-89 (3x F.grid_sample(bilinear, zeros, align_corners=False) + weighted sum).
 *      value (T) [B, L, M, D]           L = sum_l H_l*W_l, levels concatenated fine -> coarse
 *      shapes i32 [nl, 2]  (HOST pointer) (H_l, W_l)
 *      loc   f32 [B, Q, M, nl, P, 2]    sampling locations (x, y) in [0,1] image coordinates
 *      aw    f32 [B, Q, M, nl, P]       attention weights (already softmaxed over nl*P)
 *      out   (T) [B, Q, M*D]
 *      D must be a multiple of 4 (f32) / 8 (bf16) and <= 256; nl <= 8.
 */
int tamtr_msdeform_attn_fwd(const void* value, const int32_t* shapes_host, const float* loc, const float* aw, void* out,
                            int B, int L, int M, int D, int Q, int nl, int P, int dtype, void* stream);

/*      Backward: gout (T) [B,Q,M*D] -> gvalue f32 [B,L,M,D] (ACCUMULATED with float atomics: caller zeroes it),
 *      gloc f32 [B,Q,M,nl,P,2], gaw f32 [B,Q,M,nl,P].
 */
int tamtr_msdeform_attn_bwd(const void* gout, const void* value, const int32_t* shapes_host, const float* loc,
                            const float* aw, float* gvalue, float* gloc, float* gaw, int B, int L, int M, int D, int Q,
                            int nl, int P, int dtype, void* stream);

/*      Backward without atomics: the same gloc / gaw, and gvalue (T, the VALUE's dtype) written exactly once per element as an
 *      ordered sum - the caller neither zeroes it nor casts it, and two calls on the same inputs give the same bits (the
 *      reference trains with deterministic=True: ultralytics/cfg/default.yaml:26, utils/torch_utils.py:371-389; torch's own
 *      grid_sample backward is the atomic scatter this replaces).  Per (image, head, level) the Q*P*4 bilinear corners are sorted
 *      by destination row in LDS and every row sums its run.  gvalue rows have pitch ldg elements (M*D for a plain [B,L,M,D]
 *      tensor).  Limits: Q*P*4 <= 8192, D % 8 == 0, D <= 256, H*W < 2^19 - 1 per level; TAMTR_EUNSUP otherwise.
 *      colw f32 [B, Q, M] or NULL (ABI 34): per (image, query, head) the total weight it put ON the map - the sum over levels, points
 *      and the corners that lie on the map of aw * bilinear weight (1 when no corner falls off).  The column sums of gvalue over
 *      its B*L rows are then sum_{b,q} gout[b,q,m,:] * colw[b,q,m]: the bias gradient of the linear layer that produced `value`
 *      (MSDeformAttn.value_proj, nn/modules/transformer.py:273-275) from Q-sized operands, without a pass over the 550 MB gvalue.
 */
int tamtr_msdeform_attn_bwd_sorted(const void* gout, const void* value, const int32_t* shapes_host, const float* loc,
                                   const float* aw, void* gvalue, float* gloc, float* gaw, float* colw, int B, int L, int M,
                                   int D, int Q, int nl, int P, long long ldg, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * a-8  Text-contrastive logits.  Replaces ContrastiveHeadMLP.forward, ultralytics/nn/modules/block.py:534-541:
 *          logits[b,q,k] = < x[b,q,:]/max(|x|,1e-12), w[b,k,:]/max(|w|,1e-12) > * exp(logit_scale) + bias
 *      x (T) [B,Q,C]; w f32 [B,K,C]; logit_scale, bias: f32 device scalars; logits f32 [B,Q,K];
 *      xinv f32 [B,Q], winv f32 [B,K]: saved reciprocal norms (for _bwd).   C % 64 == 0, C <= 2048, K <= 128.
 */
int tamtr_contrastive_logits_fwd(const void* x, const float* w, const float* logit_scale, const float* bias, float* logits,
                                 float* xinv, float* winv, int B, int Q, int K, int C, int dtype, void* stream);

/*      Backward: g f32 [B,Q,K] -> dx (T) [B,Q,C], dwhat f32 [B, S, K, C] with S = tamtr_contrastive_bwd_slabs(Q): every
 *      workgroup STORES the partial sum of its query rows into its own slab (no atomics between workgroups; for K <= 16 none
 *      inside either, so the result is bitwise reproducible); the caller adds the S slabs.  The sum is the gradient w.r.t. the
 *      *normalised* text rows, which the host projects through the normalisation - a [B,K,C] elementwise op.
 */
int tamtr_contrastive_bwd_slabs(int Q);
int tamtr_contrastive_logits_bwd(const float* g, const void* x, const float* w, const float* logit_scale, const float* xinv,
                                 const float* winv, void* dx, float* dwhat, int B, int Q, int K, int C, int dtype,
                                 void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * a-5  MEH cross-attention value projection (the dominant dense contraction, M = B*L = 537 600 at 640^2 bs 16).
 *      Replaces `value = self.value_proj(value)`, ultralytics/nn/modules/transformer.py:273 (nn.Linear(512,512)),
 *      and any other y = x @ W^T + b of the head with N, K multiples of 128/64:
 *          Y[M,N] = X[M,K] @ W[N,K]^T + bias[N]        bf16 in, fp32 MFMA accumulate, bf16 out
 *      X bf16 [M,K] row-major, W bf16 [N,K] row-major (nn.Linear layout), bias f32 [N] or NULL, Y bf16 [M,N].
 *      Requires K % 64 == 0, N % 128 == 0; any M >= 1; X, W, Y and bias 16-byte aligned (4 bytes do for the bias
 *      where K is 128, 256 or 512 and N / 256 divides 32); TAMTR_EUNSUP otherwise, before any launch.
 */
int tamtr_linear_bf16(const void* X, const void* W, const float* bias, void* Y, int M, int N, int K, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * a-7  Small-Q masked multi-head self-attention core.  Replaces the attention inside nn.MultiheadAttention as called
 *      at ultralytics/nn/modules/transformer.py:546 (after the packed in-projection, before out_proj):
 *          O[b,:,h,:] = softmax( Qh Kh^T / sqrt(dh) + mask ) Vh
 *      q,k,v (T): row (b, i) of head h starts at ptr + (b*Q + i)*ld + h*dh  (ldq/ldk/ldv in elements, multiples of 4:
 *      views into the packed in-projection output need no copy); mask_bits u32 [Q, ceil(Q/32)] or NULL, bit j%32 of word
 *      j/32 of row i set = query i may NOT attend to key j; o (T) [B,Q,nh*dh] contiguous; lse f32 [B,nh,Q] saved
 *      log-sum-exp.  dh in {32, 64}, Q <= 4096.
 */
int tamtr_selfattn_fwd(const void* q, const void* k, const void* v, const uint32_t* mask_bits, void* o, float* lse, int B,
                       int Q, int nh, int dh, int ldq, int ldk, int ldv, int dtype, void* stream);
/*      Backward: go (T) [B,Q,nh*dh] -> gq, gk, gv (T) [B,Q,nh*dh] contiguous; delta_ws f32 [B,nh,Q] caller workspace. */
int tamtr_selfattn_bwd(const void* go, const void* q, const void* k, const void* v, const void* o, const float* lse,
                       const uint32_t* mask_bits, void* gq, void* gk, void* gv, float* delta_ws, int B, int Q, int nh, int dh,
                       int ldq, int ldk, int ldv, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * a-9  Selective scan (S6), replacing the external CUDA extension selective_scan_cuda_core.fwd/bwd that the reference
 *      calls at ultralytics/nn/extra_modules/VManba/csms6s.py:257,267 (contract: vmamba.py:962-990), fp32:
 *          dt = softplus(delta + dbias);  h_t = exp(dt_t A) h_{t-1} + dt_t B_t u_t;  y_t = <C_t, h_t> + D u_t
 *      u, delta f32 [B, KD, L]; A f32 [KD, N]; Bm, Cm f32 [B, K, N, L]; D, dbias f32 [KD]; y f32 [B, KD, L].
 *      N == 16.  hstate f32 [B, KD, nchunk, N]: state checkpoints saved for _bwd (the state after every `chunk` steps),
 *      nchunk = ceil(L / chunk) with `chunk` returned by tamtr_selective_scan_chunk() (64 since ABI 23).
 *      xmode = 0: plain contract above.  xmode = 1 ("cross-scan layout", K must be 4; replaces the 4x materialisation of
 *      CrossScan, csms6s.py:4-14): u is [B, 2, Dk, L] = (row-major, column-major) flattenings of the map, direction k reads
 *      u[:, k & 1]; directions k >= 2 are the reversed scans and walk EVERY time-indexed buffer (u, delta, B, C, y and the
 *      gradients) back to front, i.e. those buffers are stored in the un-reversed order of direction k - 2.
 */
int tamtr_selective_scan_chunk(void);
int tamtr_selective_scan_fwd(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm,
                             const float* D, const float* dbias, float* y, float* hstate, int B, int K, int Dk, int N, int L,
                             int xmode, void* stream);
/*      Backward: gy f32 [B,KD,L] -> gu, gdelta f32 [B,KD,L] (in xmode gu is per direction, stored un-reversed: the host adds
 *      gu[:, k] + gu[:, k+2] to get the gradient of u[:, k]); gB, gC f32 [B,K,N,L] (plain stores);
 *      grow f32 [B, KD, S], S = tamtr_selective_scan_row_sums() (= 64): per image and row the sums over time
 *          grow[b, kd, 0:16] = dA[kd, :] | [16:16+R] = d(Wdt)[kd, :] (dtproj variant) | [48] = dD[kd] | [49] = d(dbias)[kd]
 *      written with plain stores (one writer per (b, kd)); the caller adds the B images - in a fixed order, so the result is bitwise
 *      reproducible (ABI <= 21 accumulated gA / gD / gdbias / gWdt over the batch with float atomics).  ws: caller workspace of
 *      2 * tamtr_selective_scan_bwd_slabs(Dk) * B*K*N*L floats (per-workgroup partial dB/dC slabs, summed in slab order by a second
 *      kernel; the dtproj variant reuses it for the row-split partials of gdtr on short sequences).
 *      xmode = 3 (backward only): as xmode = 1 and gy is ALSO in pair layout [B, 2, Dk, L] - the gradient of the
 *      cross-merged map (CrossMerge, csms6s.py:26-34) in its row-major and column-major flattening; direction k reads
 *      gy[:, k & 1], so the four per-direction gradient planes are never materialised.
 */
int tamtr_selective_scan_bwd_slabs(int Dk);
int tamtr_selective_scan_row_sums(void);
int tamtr_selective_scan_bwd(const float* gy, const float* u, const float* delta, const float* A, const float* Bm,
                             const float* Cm, const float* D, const float* dbias, const float* hstate, float* gu,
                             float* gdelta, float* grow, float* gB, float* gC, float* ws, int B, int K, int Dk, int N, int L,
                             int xmode, void* stream);

/*      Fused dt projection (replaces the `dts = einsum("bkrl,kdr->bkdl")` of SS2D.forward_corev2, vmamba.py:972, whose
 *      [B, 4*d_inner, L] result is never materialised): delta[b, k*Dk+d, t] = sum_r Wdt[k*Dk+d, r] * dtr[b, k, r, t] is formed
 *      inside the scan.  dtr f32 [B, K, R, L], Wdt f32 [KD, R], R <= 32.  Backward additionally returns gdtr f32 [B,K,R,L]
 *      (plain stores) and d(Wdt) inside grow (see above); gdelta_ws: caller workspace [B,KD,L] - f32, or bf16 with ws_bf16 = 1 (L % 4 == 0):
 *      d(delta) is only the operand of gdtr = Wdt^T d(delta) there, so in bf16 mode - where the caller rounds gdtr to bf16 anyway - the
 *      workspace, the largest buffer the backward writes and re-reads, can be half the size.
 *      bf16 PLANES (bf16 mode, L % 4 == 0): with planes_bf16 = 1 (forward) / bit 1 of bf16_flags (backward; bit 0 = the d(delta) workspace
 *      above, required with it) the big time-indexed operands that cross HBM - u and y in the forward; gy, u and gu in the backward - are
 *      bf16 arrays of the same shapes.  The recurrence, the states, the checkpoints, dtr / B / C and every gradient sum stay f32: only the
 *      1.7 GB planes of a level are narrowed (what torch autocast makes of `u` anyway: the depthwise convolution's output is bf16 there).
 */
int tamtr_selective_scan_dtproj_fwd(const void* u, const float* dtr, const float* Wdt, const float* A, const float* Bm,
                                    const float* Cm, const float* D, const float* dbias, void* y, float* hstate, int B, int K,
                                    int Dk, int N, int R, int L, int xmode, int planes_bf16, void* stream);
int tamtr_selective_scan_dtproj_bwd(const void* gy, const void* u, const float* dtr, const float* Wdt, const float* A,
                                    const float* Bm, const float* Cm, const float* D, const float* dbias, const float* hstate,
                                    void* gu, void* gdelta_ws, float* gdtr, float* grow, float* gB, float* gC, float* ws, int B,
                                    int K, int Dk, int N, int R, int L, int xmode, int bf16_flags, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * a-10 / next-4  Device-side Hungarian assignment.  Replaces `C.cpu()` + scipy.optimize.linear_sum_assignment per
 *      image in HungarianMatcher.forward, ultralytics/models/utils/ops.py:98-119 (and its four host syncs per step).
 *      Same solver as scipy's (shortest augmenting paths, float64 duals, same scan order and tie rule): the pairs
 *      returned are scipy's, in scipy's order (ascending query index inside each image).
 *      cost  f32 [bs, nq, G]         finite matching costs, G = sum(group_sizes); image b owns columns
 *                                    [off_b, off_b + group_sizes[b])
 *      group_sizes_host i32 [bs]     HOST array (boxes per image; bs <= 256)
 *      batch_idx/query_idx/gt_idx i64 [sum_b min(nq, group_sizes[b])]   outputs: image, query and GLOBAL box index of
 *                                    every matched pair (query_idx = gt_idx = -1 for an image whose costs are not finite)
 *      TAMTR_EUNSUP when one image needs more than 64 KB of LDS (about nq + boxes > 3000).
 */
int tamtr_lsap_assign(const float* cost, const int32_t* group_sizes_host, int bs, int nq, int G, int64_t* batch_idx,
                      int64_t* query_idx, int64_t* gt_idx, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * next-3  CPAM gates.  Replaces CPAM.forward after its max-pool, ultralytics/nn/extra_modules/block.py:271-308:
 *          c   = sigmoid(interpolate(p, scale_factor=2, mode='bilinear', align_corners=False)) * x,  p = MaxPool2d(3,2,1)(x)
 *          out = cat_g( sigmoid(max over the channels of chunk g of c) * c_g ),  g = 0..7  (c.chunk(8, 1))
 *      x, out (T) [B, C, H, W]     H, W even (odd maps make the reference fail too), C % 8 == 0
 *      p      (T) [B, C, H/2, W/2] pooled map (the caller runs the max-pool and keeps its indices for the backward)
 *      s2    f32 [B, 8, H, W]      saved sigmoid of the chunk max     } consumed by _bwd
 *      arg   i32 [B, 8, H, W]      channel (inside the chunk) holding the max }
 */
int tamtr_cpam_fwd(const void* x, const void* p, void* out, float* s2, int32_t* arg, int B, int C, int H, int W, int dtype,
                   void* stream);

/*      Backward.  gout (T) [B,C,H,W] ->
 *      dx_direct (T) [B,C,H,W]    dL/dx through the product sigmoid(up(p)) * x
 *      dp        (T) [B,C,H/2,W/2] dL/dp (caller scatters it through the max-pool indices and adds it to dx_direct)
 *      du_ws     (T) [B,C,H,W]    workspace (dL/d upsampled map) between the two kernels
 */
int tamtr_cpam_bwd(const void* gout, const void* x, const void* p, const float* s2, const int32_t* arg, void* dx_direct,
                   void* du_ws, void* dp, int B, int C, int H, int W, int dtype, void* stream);

/*      The whole op on channels-last maps (what the trunk runs), its max-pool included: x, p, out, gout, dx and the workspaces (T)
 *      [B][H][W][C] / [B][H/2][W/2][C]; code u8 [B][H/2][W/2][C]: which element of its 3 x 3 window each pooled value is (row-major position in
 *      the unclipped window; first maximum wins, NaN wins - csrc/pool.hip's rules); s2 f32 / arg i32 [B][H][W][8] (chunk innermost).
 *      A lane owns 16 bytes of channels of a pooled cell / a 2 x 2 pixel block / a pixel; the chunk max / sum is a butterfly over the chunk's
 *      lanes: C % 64 == 0 (bf16) / % 32 (f32), C / 8 a power of two times the vector width, 16-byte aligned pointers.  Forward: p, code, out,
 *      s2, arg are written (2 launches).  Backward: gout -> dx (3 launches: gates, bilinear gather into dp_ws, pool gather + direct term);
 *      dxd_ws, du_ws [B][H][W][C] and dp_ws [B][H/2][W/2][C] are caller workspaces.  No transposing copies around the op. */
int tamtr_cpam_cl_fwd(const void* x, void* p, uint8_t* code, void* out, float* s2, int32_t* arg, int B, int C, int H, int W, int dtype, void* stream);
int tamtr_cpam_cl_bwd(const void* gout, const void* x, const void* p, const uint8_t* code, const float* s2, const int32_t* arg, void* dxd_ws,
                      void* du_ws, void* dp_ws, void* dx, int B, int C, int H, int W, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * a-9  SS2D front end: depthwise 3x3 conv + bias + SiLU + cross-scan layout.  Replaces `x = self.act(self.conv2d(x))`
 *      (ultralytics/nn/extra_modules/VManba/vmamba.py:949-952, on the NCHW permutation of the in_proj output) together with
 *      CrossScan (VManba/csms6s.py:4-14) in the pair layout of tamtr_selective_scan_* (xmode = 1).
 *      x      (T) channels-last map: pixel (b, h, w) starts at x + ((b*H + h)*W + w) * x_pixel_stride, D channels are read
 *                 (the in_proj output [B, H, W, 2*d_inner] is passed as it lies, x_pixel_stride = 2*d_inner)
 *      weight f32 [D, 9] (= conv2d.weight [D, 1, 3, 3]), bias f32 [D] or NULL
 *      u2     f32 [B, 2, D, H*W]: plane 0 = SiLU(conv) flattened row-major (h*W + w), plane 1 column-major (w*H + h)
 *      D % 32 == 0; x_pixel_stride a multiple of 16 bytes.
 *      plane_dtype: TAMTR_F32, or TAMTR_BF16 (with dtype = TAMTR_BF16 only): u2 / g2 are bf16 arrays of the same shape ("bf16 PLANES",
 *      tamtr_selective_scan_dtproj_fwd).
 */
int tamtr_dwconv_silu_cross_fwd(const void* x, long long x_pixel_stride, const float* weight, const float* bias, void* u2, int B,
                                int D, int H, int W, int dtype, int plane_dtype, void* stream);
/*      Backward.  g2 f32 [B, 2, D, H*W] (gradient of u2) ->
 *      gx (T) channels-last, pixel stride gx_pixel_stride (D channels written per pixel),
 *      ws f32 [B, tamtr_dwconv_tiles(H, W), D, 10]: per-tile partial sums of d(weight) (9 taps) and d(bias) (caller sums
 *      over the first two axes; no atomics).
 */
int tamtr_dwconv_tiles(int H, int W);
int tamtr_dwconv_silu_cross_bwd(const void* g2, const void* x, long long x_pixel_stride, const float* weight, const float* bias,
                                void* gx, long long gx_pixel_stride, float* ws, int B, int D, int H, int W, int dtype, int plane_dtype,
                                void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * a-9  SS2D back end.  tamtr_cross_merge_* replace CrossMerge (VManba/csms6s.py:26-34) and the transposition to channels-last:
 *          ymT[b, h*W+w, d] = y4[b,0,d,h*W+w] + y4[b,2,d,h*W+w] + y4[b,1,d,w*H+h] + y4[b,3,d,w*H+h]
 *      y4 f32 [B, 4, D, H*W] (scan outputs, un-reversed, as tamtr_selective_scan_* with xmode = 1 write them), ymT f32 [B, H*W, D];
 *      backward: gymT f32 [B, H*W, D] -> g2 f32 [B, 2, D, H*W], the gradient in pair layout that the scan backward reads with
 *      xmode = 3.  D % 32 == 0.  plane_dtype: the element type of y4 / g2 (TAMTR_F32 | TAMTR_BF16, "bf16 PLANES"); ymT / gymT stay f32.
 */
int tamtr_cross_merge_fwd(const void* y4, float* ymT, int B, int D, int H, int W, int plane_dtype, void* stream);
int tamtr_cross_merge_bwd(const float* gymT, void* g2, int B, int D, int H, int W, int plane_dtype, void* stream);

/*      tamtr_ln_gate_* replace `y = self.out_norm(y); y = y * self.act(z)` (VManba/vmamba.py:1005-1008,1029-1036):
 *          out[t, :] = LayerNorm(x[t, :]; gamma, beta, eps) * SiLU(z[t, :]),  z[t, d] = xz[t * xz_token_stride + D + d]
 *      x f32 [ntok, D]; xz (T) the channels-last in_proj output (z = second half of each token's 2*D row); out (T) [ntok, D];
 *      stats f32 [ntok, 2] (mean, 1/std) saved for the backward.  D in {64, 128, 256, 512, 1024}.
 *      Backward: gout (T) [ntok, D] -> gx f32 [ntok, D]; d(z) written into gxz (T) at the same offsets as z in xz (the
 *      caller zero-fills the x half); partials f32 [tamtr_ln_gate_blocks(ntok), 2, D]: per-workgroup sums of d(gamma), d(beta).
 */
int tamtr_ln_gate_blocks(long long ntok);
int tamtr_ln_gate_fwd(const float* x, const void* xz, long long xz_token_stride, const float* gamma, const float* beta, void* out,
                      float* stats, long long ntok, int D, float eps, int dtype, void* stream);
int tamtr_ln_gate_bwd(const void* gout, const float* x, const void* xz, long long xz_token_stride, const float* gamma,
                      const float* beta, const float* stats, float* gx, void* gxz, float* partials, long long ntok, int D, int dtype,
                      void* stream);

/*      Gradient of the two stored cross-scan copies (SS2D backward): out[b, i] = g4[b, i] + g4[b, i + 2] + m_i[b], i = 0, 1.
 *      g4 f32 [B, 4, n] = d/d(u) of the four directions as tamtr_selective_scan_dtproj_bwd writes them (un-reversed), m0 / m1 (T)
 *      [B, n] = the x_proj backward products of the two copies (vmamba.py:962-970), out f32 [B, 2, n], n = D * L, n % 4 == 0.
 */
/*      out = src[0] + ... + src[n-1] (n <= 8 tensors of n_elems elements, T; src: HOST array of device pointers): the gradient of a
 *      tensor with several consumers - the MEH token memory feeds enc_output and every decoder layer's value_proj (head.py:1152-1160,
 *      transformer.py:273) - in one pass instead of autograd's n - 1 pairwise adds. */
int tamtr_sum_n(const void* const* src, int n, void* out, long long n_elems, int dtype, void* stream);

/*      Column sums of a tall bf16 matrix: the bias gradient of a token-wise nn.Linear (value_proj transformer.py:273, enc_output
 *      head.py:1118: db = sum over the B*L tokens of dY).  X bf16 [M, N] -> partial f32 [tamtr_colsum_blocks(M), N], one row of sums per
 *      workgroup, added by the caller (fixed order).  N % 8 == 0, N <= 2048, 256 % (N / 8) == 0. */
int tamtr_colsum_blocks(long long M);
int tamtr_colsum_bf16(const void* X, float* partial, long long M, int N, void* stream);
/*      out f32 [C] = sum over the R rows of in (T) [R, C], added in a fixed order in ONE launch: the last stage of the package's two-stage
 *      reductions - the d(gamma) / d(beta) partial rows of LayerNorm (vmamba.py:1190,1222 backward), the depthwise convolution's
 *      d(weight) tile sums (vmamba.py:949-952), the scan's per-image d(A) / d(D) rows (csms6s.py:267), the row-slice products of the
 *      tall linears' weight gradients (vmamba.py:935,1010 in_proj / out_proj).  Stands where `partials.sum(0)` stood: torch's
 *      multi-workgroup reduction zeroes a semaphore buffer with a memset node per launch, which a HIP-graph replay under AQL packet
 *      capture does not keep in order with the kernels around it.  C % 4 == 0; in 16-byte (f32) / 8-byte (bf16) aligned. */
int tamtr_slab_sum_rows(const void* in, float* out, int R, long long C, int dtype, void* stream);
/*      Weight (and bias) gradient of a token-wise linear or 1x1 convolution for SHORT and MID-SIZE M, as row-slice partials
 *      (csrc/dwgrad.hip):  part[s][n * K + k] = sum over the rows m of slice s of dY[m, n] X[m, k];  part[s][N * K + n] = the slice's
 *      column sums of dY (with_db) or 0.  dY bf16 [M, N], X bf16 [M, K], part f32 [S][N * K + Npad] (Npad = N rounded up to 4), all
 *      contiguous and 16-byte aligned; S = tamtr_dw_slices(M, N, K) (host only, 1 .. 64; 0: shape not served - N, K multiples of 16 up
 *      to 16 384, any M >= 1).  Slice s covers rows [s * R, min(M, (s + 1) * R)) with R = ceil(ceil(M / S) / 64) * 64.  One kernel,
 *      plain stores, every element of part written once: no atomics, no memset.  The caller adds the S rows in order
 *      (tamtr_slab_sum_rows: dW and db in one launch); bf16 MFMA with fp32 accumulators, the column sums in fp32 in a fixed order. */
int tamtr_dw_slices(long long M, int N, int K);
int tamtr_dw_bf16(const void* dY, const void* X, float* part, int with_db, long long M, int N, int K, void* stream);
int tamtr_fold_add(const float* g4, const void* m0, const void* m1, float* out, int B, long long n, int dtype, void* stream);

/*      tamtr_layernorm_* : LayerNorm over the channel axis of a token-major map, VSSBlock.norm / norm2
 *      (VManba/vmamba.py:1190,1222,1239-1254).  x, out, gout, gx (T) [ntok, D]; gamma, beta f32 [D]; stats f32 [ntok, 2];
 *      partials f32 [tamtr_ln_gate_blocks(ntok), 2, D] (per-workgroup d(gamma), d(beta) sums).  D in {32,...,1024} powers of two.
 */
int tamtr_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* out, float* stats, long long ntok, int D,
                        float eps, int dtype, void* stream);
int tamtr_layernorm_bwd(const void* gout, const void* x, const float* gamma, const float* stats, void* gx, float* partials,
                        long long ntok, int D, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * trunk  Training-mode BatchNorm2d (+ SiLU).  Replaces `self.act(self.bn(y))` of Conv.forward, ultralytics/nn/modules/conv.py:36-40,
 *      in train mode (batch statistics, running-stat update with the unbiased variance, as nn.BatchNorm2d).
 *      x, y, gy, gx (T) [B, C, HW] (NCHW maps); gamma, beta, running_mean, running_var f32 [C] (running_* may be NULL);
 *      mean_rstd f32 [C, 2] saved for the backward; partials: caller workspace of C * tamtr_bn_slices(B, HW) * 3 floats
 *      (forward) / * 2 floats (backward).  act: 0 = identity, 1 = SiLU.  Backward returns d(gamma), d(beta) f32 [C].
 */
int tamtr_bn_slices(int B, int HW);
int tamtr_bn_act_fwd(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var, void* y,
                     float* mean_rstd, float* partials, int B, int C, int HW, float eps, float momentum, int act, int dtype, void* stream);
int tamtr_bn_act_bwd(const void* gy, const void* x, const float* gamma, const float* beta, const float* mean_rstd, void* gx,
                     float* ggamma, float* gbeta, float* partials, int B, int C, int HW, int act, int dtype, void* stream);

/*      Channels-last variant (token-major maps, e.g. the MEH input projection output [B*L, hd] of head.py:1087 run as a GEMM):
 *      x, y, gy, gx (T) [N, C], C contiguous and 16-byte aligned, C <= 1024, C % 4 == 0 and 256 % (C / V) == 0 with V = 8 for
 *      bf16 maps with C % 8 == 0, else 4.  partials: caller workspace of S = tamtr_bncl_blocks(N, C, dtype) chunks:
 *      C * S * 3 floats (forward) / C * S * 2 + 2 * C floats (backward).  ldgy: row pitch of gy in elements (C = packed; larger when
 *      the gradient is a channel slice of the gradient of a `torch.cat(..., 1)`, so that no packing copy is needed).
 */
int tamtr_bncl_blocks(long long N, int C, int dtype);
int tamtr_bncl_act_fwd(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var, const void* residual,
                       void* y, float* mean_rstd, float* partials, long long N, int C, float eps, float momentum, int act, int dtype,
                       void* stream);
/*      residual (T [N, C], may be NULL): y = act(bn(x)) + residual - the shortcut of RepNBottleneck (`x + self.cv2(self.cv1(x))`,
 *      extra_modules/block.py:100-102) joins in the apply pass; its gradient is gy itself (the caller passes it on).
 *      tamtr_bncl2_act_*: y = act(bn1(x1) + bn2(x2)), both in training mode over the same shape - RepConvN's training form
 *      `self.act(self.conv1(x) + self.conv2(x))` (block.py:66-69).  mean_rstd f32 [2][C][2]; partials 2 * C * S * 3 floats forward,
 *      C * S * 3 + 3 * C backward.
 */
int tamtr_bncl_stats(const void* x, float* running_mean, float* running_var, float* mean_rstd, float* partials, long long N, int C, float eps,
                     float momentum, int dtype, void* stream);   /* batch statistics + running update only: mean_rstd f32 [C][2] */
int tamtr_bncl2_act_fwd(const void* x1, const float* gamma1, const float* beta1, float* running_mean1, float* running_var1, const void* x2,
                        const float* gamma2, const float* beta2, float* running_mean2, float* running_var2, void* y, float* mean_rstd,
                        float* partials, long long N, int C, float eps, float momentum, int act, int dtype, void* stream);
int tamtr_bncl2_act_bwd(const void* gy, long long ldgy, const void* x1, const void* x2, const float* gamma1, const float* beta1,
                        const float* gamma2, const float* beta2, const float* mean_rstd, void* gx1, void* gx2, float* ggamma1, float* gbeta1,
                        float* ggamma2, float* gbeta2, float* partials, long long N, int C, int act, int dtype, void* stream);
int tamtr_bncl_act_bwd(const void* gy, long long ldgy, const void* x, const float* gamma, const float* beta, const float* mean_rstd,
                       void* gx, float* ggamma, float* gbeta, float* partials, long long N, int C, int act, int dtype, void* stream);
/*      tamtr_bncl_act_down2_*: y = act(bn(x))[:, ::2, ::2] - a Conv whose only consumer is a nearest x0.5 resample (TAMTR.yaml layers 13-14,
 *      21-22, 29-30).  x, gx (T) [B, H, W, C] channels-last, H and W even; y, gy (T) [B, H/2, W/2, C] (gy with row pitch ldgy).  The batch
 *      statistics, mean_rstd and the running update are those of tamtr_bncl_act_fwd over all N = B * H * W rows; the apply pass and the
 *      backward reduction read the kept pixels only, and gx is written at every pixel.  The backward sums (hence ggamma, gbeta, gx) have the
 *      bits tamtr_bncl_act_bwd gives for gy scattered into a zero full map.  partials: C * S * 3 floats forward, C * S * 2 + 2 * C floats
 *      backward, S = tamtr_bncl_blocks(N, C, dtype).
 */
int tamtr_bncl_act_down2_fwd(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var, void* y,
                             float* mean_rstd, float* partials, int B, int H, int W, int C, float eps, float momentum, int act, int dtype,
                             void* stream);
int tamtr_bncl_act_down2_bwd(const void* gy, long long ldgy, const void* x, const float* gamma, const float* beta, const float* mean_rstd,
                             void* gx, float* ggamma, float* gbeta, float* partials, int B, int H, int W, int C, int act, int dtype,
                             void* stream);

/* ---- layout: NCHW <-> NHWC repacking of a feature map (tiled transpose through LDS).  The trunk runs channels-last around
 *      MIOpen's NHWC convolutions; the gate (a-1) and CPAM (next-3) kernels read NCHW planes.  Replaces torch's
 *      `.contiguous()` / `.contiguous(memory_format=torch.channels_last)` on those edges (same values, no arithmetic).
 *      to_nhwc != 0: src [B, C, HW] -> dst [B, HW, C];  to_nhwc == 0: src [B, HW, C] -> dst [B, C, HW].  T = f32 | bf16.
 *      ld: pixel pitch of the NHWC side in elements (ld == C: packed; ld > C: a channel slice of a wider map, e.g. one half of
 *      `cv1(x).chunk(2, 1)`, extra_modules/block.py:147).
 */
int tamtr_relayout(const void* src, void* dst, int B, int C, int HW, int ld, int to_nhwc, int dtype, void* stream);
/*      Channel-slice copy on channels-last maps: dst[r][0..C) = src[r][0..C), N = B*H*W rows, row pitches lds / ldd elements.
 *      Replaces the strided copies behind `torch.cat(y, 1)` / `x.chunk(2, 1)` (extra_modules/block.py:133,147,152) in NHWC. */
/*      Nearest-neighbour x2 / x0.5 resampling of a packed NHWC map = nn.Upsample(scale_factor=2.0 | 0.5, mode='nearest') as TAMTR.yaml
 *      uses it, forward and backward.  mode 0: dst [B,2H,2W,C] <- src [B,H,W,C] (up);  1: dst [B,H,W,C] <- src [B,2H,2W,C] (its
 *      gradient: sum of the four);  2: dst [B,H/2,W/2,C] <- src [B,H,W,C] (down: every second pixel);  3: dst [B,H,W,C] <- src
 *      [B,H/2,W/2,C] (its gradient: scattered, zeros elsewhere, one pass).  C % 8 == 0 (bf16) / C % 4 == 0 (f32). */
int tamtr_resample2(const void* src, void* dst, int B, int H, int W, int C, int mode, int dtype, void* stream);
int tamtr_copy_rows(const void* src, long long lds, void* dst, long long ldd, long long N, int C, int dtype, void* stream);
/*      The whole `torch.cat(y, 1)` of up to four channels-last maps in one launch: dst[r][off_k .. off_k + C[k]) = src[k][r][0 .. C[k]),
 *      off_k = C[0] + ... + C[k-1]; src / lds / C are HOST arrays of n <= 4 entries (pointers are device pointers); widths, pitches
 *      and pointers 16-byte granular, else TAMTR_EUNSUP (then copy input by input). */
int tamtr_cat_rows(const void* const* src, const long long* lds, const int* C, int n, void* dst, long long ldd, long long N, int dtype,
                   void* stream);

/* ---- max pooling k x k / stride s / padding p (floor mode), NCHW (nhwc = 0) or NHWC (nhwc = 1) maps.  Replaces nn.MaxPool2d as
 *      used by SPPELAN (5/1/2, three chained: ultralytics/nn/extra_modules/block.py:255-268) and by CPAM's channel gate (3/2/1,
 *      block.py:274), forward and backward.  code: one byte per output element = position of the winner inside the unclipped
 *      window (row-major; first maximum wins, NaN wins over everything - torch's rule).  The backward gathers (no atomics).
 *      addend (T, same layout as gx, may be NULL): gx = addend + pooled gradient (CPAM adds its direct term this way).
 *      x, gx (T) [B,C,H,W] in the given layout; y, gy (T) and code (u8) [B,C,Ho,Wo], Ho = tamtr_maxpool_out(H, k, s, p).  k <= 15.
 */
int tamtr_maxpool_out(int n, int k, int s, int p);
int tamtr_maxpool_fwd(const void* x, void* y, uint8_t* code, int B, int C, int H, int W, int k, int s, int p, int nhwc, int dtype,
                      void* stream);
int tamtr_maxpool_bwd(const void* gy, const uint8_t* code, const void* addend, void* gx, int B, int C, int H, int W, int k, int s, int p, int nhwc, int dtype,
                      void* stream);

/* ---- data path: the pixel half of the training transforms on the device.
 *      Replaces, for a whole batch and in this order: cv2.warpAffine(img, M[:2], dsize, borderValue=114) of RandomPerspective
 *      (ultralytics/data/augment.py:415-420), the BGR2HSV -> LUT -> HSV2BGR chain of RandomHSV (:590-609), RandomFlip's
 *      np.flipud / np.fliplr (:656-660), Format._format_img (:920-926) and preprocess_batch's img.float() / 255
 *      (models/yolo/detect/train.py:56).  Same arithmetic as libtamtr_host.so (include/tamtr_host.h), bit for bit.
 *      src        u8  [B, SH, SW, 3]  decoded + stretched RGB images (before any transform)
 *      inv_affine f64 [B, 6]          destination -> source map  m0 m1 b1 / m3 m4 b2  (inverse of the transform's 2x3 matrix)
 *      luts       u8  [B, 3, 256]     hue (< 180), saturation, value look-up tables of RandomHSV
 *      flags      i32 [B]             bit 0: flipped up-down, bit 1: flipped left-right, bit 2: no HSV step (luts ignored)
 *      out        f32 [B, 3, H, W]    pixel * float(1 / 255.0), which is how torch evaluates `img.float() / 255` on the device
 */
int tamtr_img_augment_u8(const uint8_t* src, const double* inv_affine, const uint8_t* luts, const int32_t* flags, float* out, int B,
                         int SH, int SW, int H, int W, int border, void* stream);

/*      The reference's optimizer_step (ultralytics/engine/trainer.py:471-479): clip_grad_norm_(max_norm) -> AdamW.step() ->
 *      ModelEMA.update (utils/torch_utils.py:392-419), over a device table of tensors built once by the caller; torch's FusedAdamKernel
 *      arithmetic in fp32.  All table arrays are DEVICE arrays with one entry per tensor unless noted:
 *        p, m, v, e   addresses of the values, exp_avg, exp_avg_sq and EMA copy (m[i] == 0: EMA-only entry, e.g. BatchNorm statistics;
 *                     e[i] == 0: no EMA), all f32 with the element order of p;  step f32: Adam step counts (advanced for tensors that have a
 *                     gradient);  numel i64;  group u8: parameter group;  chunk_tensor i32 / chunk_off i64 [nchunks]: the tensors cut into
 *                     pieces of tamtr_optim_chunk() elements;  grads: THIS step's gradient addresses (0: none - Adam skipped, EMA still taken).
 *        partial f32 [nchunks], normcoef f32 [2] workspaces; normcoef = {total gradient norm, clip coefficient} afterwards (device side:
 *                     nothing is read back).  lr, wd: HOST arrays [ngroups <= 4].  max_norm <= 0: no clipping.  do_ema == 0: EMA untouched.
 *      The clipped gradient is written back to the gradient buffers, as clip_grad_norm_ leaves it.
 *        shadow       NULL, or a device array of addresses of bf16 arrays with the element order of p (0: none): the updated value of every
 *                     tensor that has a gradient this step is ALSO stored there rounded to bf16 - the compute copy that bf16 autocast casts out
 *                     of the fp32 master at every use (trainer.py:343 `torch.cuda.amp.autocast`); engine.FusedOptimStep(shadows=True). */
int tamtr_optim_chunk(void);
int tamtr_optim_step(const void* const* p, const void* const* m, const void* const* v, const void* const* e, const void* const* shadow, float* step,
                     const long long* numel,
                     const unsigned char* group, const int* chunk_tensor, const long long* chunk_off, const void* const* grads, int ntensors,
                     int nchunks, float* partial, float* normcoef, const float* lr, const float* wd, int ngroups, float beta1, float beta2, float eps,
                     float max_norm, float ema_decay, int do_ema, void* stream);

/*      x_proj of SS2D on the cross-scan pair layout (ultralytics/nn/extra_modules/VManba/vmamba.py:962-975: x_dbl = einsum("b k d l, k c d
 *      -> b k c l", xs, x_proj_weight); dts, Bs, Cs = split(x_dbl, [R, N, N])), bf16 MFMA products on f32 operands as the scan kernels keep
 *      them (values rounded to bf16 in registers, products rounded to bf16 before they are stored / added: the arithmetic of the bf16
 *      library GEMMs these kernels replace).  C = R + 32, N = 16 states, 1 <= R <= 32, 2C in {66 .. 128}.
 *        u2    f32 [B, 2, D, L]     SiLU(dwconv(x)) row-major / column-major (tamtr_dwconv_silu_cross_fwd); directions k, k + 2 read copy k & 1
 *        wcat  bf16 [2, MP, D]      rows [W_i ; W_(i+2)] of x_proj_weight [4, C, D], zero-padded to MP = ceil(2C / 32) * 32 rows
 *        dtr   f32 [B, 4, R, L], Bs, Cs f32 [B, 4, 16, L]   un-reversed, as tamtr_selective_scan_dtproj_* take them
 *      backward:  gdtr, gB, gC f32 as the scan backward writes them; gu f32 [B, 4, D, L] = the scan's d/d(u) per direction;
 *        wT    bf16 [2, D, KP]      wcat transposed, zero-padded to KP = ceil(2C / 16) * 16 columns
 *        gu2   f32 [B, 2, D, L]   = gu[:, i] + gu[:, i + 2] + Wcat_i^T G_i: the gradient of the two stored copies (what tamtr_fold_add + the
 *                                   product did in two passes)
 *        part  f32 [B * tamtr_xproj_dw_slices(L), 2, 2C, D]   per-(image, 1 024-pixel slice) partial dWcat tiles; the caller adds them in
 *                                   order (tamtr_slab_sum_rows) and re-splits rows [0, C) / [C, 2C) of copy i into directions i / i + 2
 *      D % 16 == 0 (fwd), % 32 (dx), % 256 and L % 8 == 0 (dw); wcat / wT 16-byte aligned.
 *      plane_dtype = TAMTR_BF16 ("bf16 PLANES"): u2, gu and gu2 are bf16 arrays of the same shapes (L % 2 == 0); a lane then handles a pixel
 *      PAIR (one dword), a wave 64 pixels; dtr / Bs / Cs / gdtr / gB / gC / part stay f32. */
int tamtr_xproj_dw_slices(int L);
int tamtr_xproj_fwd(const void* u2, const void* wcat, float* dtr, float* Bs, float* Cs, int B, int D, int L, int R, int plane_dtype, void* stream);
int tamtr_xproj_bwd_dx(const void* gu, const float* gdtr, const float* gB, const float* gC, const void* wT, void* gu2, int B, int D, int L, int R,
                       int plane_dtype, void* stream);
int tamtr_xproj_bwd_dw(const void* u2, const float* gdtr, const float* gB, const float* gC, float* part, int B, int D, int L, int R, int plane_dtype,
                       void* stream);

/*      The per-layer terms of the RT-DETR loss and the matcher's cost matrix (a-10: ultralytics/models/utils/loss.py:85-166,282-326 - varifocal
 *      class loss on the matched IoU, 5 x L1, 2 x (1 - RIOU); RIOU: ultralytics/utils/metrics.py:91-130; cost: models/utils/ops.py:84-112), all
 *      decoder layers of a call stacked, fp32.  pb f32 [Lr, B, nq, 4] (xywh), ps f32 [Lr, B, nq, nc] (logits), gt_bboxes f32 [G, 4], gt_cls i64 [G];
 *      matched pairs as flat i64 lists li, bi, si, gi [Lr * n] (layer-major, exactly n pairs per layer, a query matched at most once per layer).
 *      fwd: workspaces tgt i64 [Lr, B, nq] PRESET to nc (no object), score f32 [Lr, B, nq] PRESET to 0, pair_l1 / pair_riou f32 [Lr * n],
 *           partial f32 [Lr * tamtr_detr_blocks(B * nq)];  out f32 [3, Lr] = (class, bbox, giou) terms, gains and 1 / n applied.
 *      bwd: up f32 [3, Lr] upstream gradients of `out`; gps f32 [Lr, B, nq, nc] (every element written), gpb f32 [Lr, B, nq, 4] (the matched rows
 *           written: the caller zero-fills).  RIOU's alpha is a constant (torch.no_grad in the reference); ties of max / min split the gradient.
 *      match_cost: C f32 [rows = Lr * B * nq, G] = g_class (focal pos - neg) + g_bbox L1 + g_giou (1 - RIOU), non-finite -> 0. */
int tamtr_detr_blocks(int rows_per_layer);
int tamtr_detr_layers_fwd(const float* pb, const float* ps, const float* gt_bboxes, const long long* gt_cls, const long long* li, const long long* bi,
                          const long long* si, const long long* gi, int Lr, int B, int nq, int nc, int n, long long* tgt, float* score, float* pair_l1,
                          float* pair_riou, float* partial, float g_class, float g_bbox, float g_giou, float* out, void* stream);
int tamtr_detr_layers_bwd(const float* pb, const float* ps, const float* gt_bboxes, const long long* li, const long long* bi, const long long* si,
                          const long long* gi, const long long* tgt, const float* score, const float* up, int Lr, int B, int nq, int nc, int n,
                          float g_class, float g_bbox, float g_giou, float* gpb, float* gps, void* stream);
int tamtr_detr_match_cost(const float* ps, const float* pb, const float* gt_bboxes, const long long* gt_cls, long long rows, int nc, int G, float g_class,
                          float g_bbox, float g_giou, float alpha, float gamma, float* C, void* stream);

/*      tamtr_bncl_act_fwd / _bwd with the OUTPUT (forward) / the incoming GRADIENT (backward) laid out as image segments of a wider buffer:
 *      level i of the MEH token memory `feats` [B, L_0 + L_1 + L_2, hd] is the BatchNorm of its input projection written straight into
 *      feats[:, off_i : off_i + L_i] (ultralytics/nn/modules/head.py:1087,1202-1219: `input_proj[i]` ... `torch.cat(feats, 1)`), and the
 *      backward reads d(feats)[:, off_i : off_i + L_i] where it lies - no concatenation copy, no slice copies.
 *      x (T) [N = B * seg_rows, C] packed; y / gy point at image 0's first row of the segment, image b's rows start b * seg_pitch elements
 *      further (seg_pitch = (L_0 + L_1 + L_2) * C); C a power of two; everything else as tamtr_bncl_act_fwd / _bwd. */
int tamtr_bncl_act_seg_fwd(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var, void* y, long long seg_rows,
                           long long seg_pitch, float* mean_rstd, float* partials, long long N, int C, float eps, float momentum, int act, int dtype,
                           void* stream);
int tamtr_bncl_act_seg_bwd(const void* gy, long long seg_rows, long long seg_pitch, const void* x, const float* gamma, const float* beta,
                           const float* mean_rstd, void* gx, float* ggamma, float* gbeta, float* partials, long long N, int C, int act, int dtype,
                           void* stream);

/*      The decoder's iterative box refinement (ultralytics/nn/modules/transformer.py:881-887, nn/modules/utils.py:46-52):
 *          out = sigmoid(delta + inverse_sigmoid(ref)),  inverse_sigmoid(x) = log(max(clamp(x, 0, 1), 1e-5) / max(1 - clamp(x, 0, 1), 1e-5))
 *      delta, ref, out f32 [n] (any shape, contiguous).  Backward: gdelta = gout out (1 - out); gref (NULL: not wanted - the reference detaches
 *      `ref` between layers) = gdelta * d(inverse_sigmoid)/d(ref) with torch's clamp gradients. */
int tamtr_box_refine_fwd(const float* delta, const float* ref, float* out, long long n, void* stream);
int tamtr_box_refine_bwd(const float* gout, const float* out, const float* ref, float* gdelta, float* gref, long long n, void* stream);

/*      Node census of the graph that `stream` is capturing into (hipStreamGetCaptureInfo_v2 + hipGraphGetNodes): counts[t] = nodes of
 *      hipGraphNodeType t, t < n_types <= 16 (0 kernel, 1 memcpy, 2 memset, ...).  Host-side helper of the HIP-graph replay
 *      (tam-tr_amd/graphs.py: memset nodes do not survive AQL packet capture); TAMTR_EINVAL when the stream is not capturing. */
int tamtr_graph_capture_census(void* stream, int* counts, int n_types);

/* ---------------------------------------------------------------------------------------------------------------
 * Predictor postprocess.  Replaces the per-image loop of RTDETRPredictor.postprocess,
 * ultralytics/models/rtdetrworld/predict.py:34-78 (xywh2xyxy, utils/ops.py:360-380; class max; `score > conf` and the
 * optional class filter; torchvision.ops.nms on boxes shifted by cls * max_wh; boxes scaled to the original image):
 *      preds   (T) [B, nq, nd]  eval output of the model: normalised cx cy w h, then nc = nd - 4 class scores; widened to fp32
 *      orig_hw i32 [B, 2]       original image (h, w) of every image
 *      classes i32 [n_classes]  class-id filter; NULL = every class (non-NULL with n_classes == 0 keeps nothing, as the reference)
 *      out     f32 [B, nq, 6]   kept rows in NMS order: x1 y1 x2 y2 (pixels of the original image), score, cls; zero after counts[b]
 *      keep    i32 [B, nq]      source query of each kept row, -1 after counts[b]
 *      counts  i32 [B]          rows kept per image
 *  Bit-exact with that rule in fp32, every operation rounded on its own; equal scores keep ascending query order (stable sort); the
 *  IoU is torchvision's (no eps: 0/0 = NaN does not suppress) on the shifted boxes (shift 0 when single_cls), a row is suppressed when
 *  IoU > iou compared in fp32 (csrc/predict.hip states how the Python op reproduces torchvision's double comparison).  One launch,
 *  one workgroup per image; nothing is allocated, set or synchronised, so the call can be captured.
 *  TAMTR_EINVAL: a NULL operand, B < 1, nq < 1, nd < 5, n_classes < 0, dtype not F32 / BF16.  TAMTR_EUNSUP: nq > 512. */
int tamtr_detect_postprocess(const void* preds, int dtype, int B, int nq, int nd, const int32_t* orig_hw, float conf, float iou,
                             int single_cls, float max_wh, const int32_t* classes, int n_classes, float* out, int32_t* keep,
                             int32_t* counts, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Validator postprocess and label matching.  Replaces the per-image loop of the validator: RTDETRValidator.postprocess,
 * ultralytics/models/rtdetrworld/val.py:102-173 (boxes scaled by imgsz, xywh2xyxy, class max, descending-score order, the confidence
 * mask, torchvision.ops.nms on boxes shifted by cls * max_wh, predictions and labels scaled to the original image), and
 * match_predictions / _process_batch, ultralytics/engine/validator.py:208-247 (IoU of labels and detections, one detection per label at
 * each of the ten thresholds 0.5 : 0.05 : 0.95):
 *      preds   (T) [B, nq, nd]  eval output of the model: normalised cx cy w h, then nc = nd - 4 class scores; widened to fp32
 *      lab_cls f32 [M]          label classes, grouped by image (file order inside an image)
 *      lab_box f32 [M, 4]       label boxes, normalised cx cy w h, same order
 *      lab_off i32 [B + 1]      image b owns labels lab_off[b] .. lab_off[b + 1] - 1 (clamped to 0 .. M); an image may own none
 *      scale   f32 [B, 4]       per image: fp32(w_orig / imgsz), fp32(h_orig / imgsz) (predictions), fp32(w_orig), fp32(h_orig) (labels)
 *      predn   f32 [B, nq, 6]   kept rows in NMS order: x1 y1 x2 y2 (pixels of the original image), score, cls; zero after counts[b]
 *      correct u8  [B, nq, 10]  row d is a true positive at threshold t; zero after counts[b]
 *      counts  i32 [B]          rows kept per image
 *  Bit-exact in fp32, every operation rounded on its own, with engine.postprocess + engine.process_batch on CPU fp32 tensors:
 *  b = xywh * imgsz before the corner conversion; rows in descending score order, stable (equal scores: ascending query; NaN first);
 *  sorted position p survives iff the score of QUERY p exceeds conf (the reference's unsorted mask on sorted rows, kept on purpose);
 *  NMS as tamtr_detect_postprocess (IoU > iou in fp32; csrc/valmatch.hip states how the Python op reproduces torchvision's double
 *  comparison and where engine.nms differs); cls = 0 when single_cls (label classes are not zeroed); matching IoU =
 *  inter / (((area_label + area_det) - inter) + fp32(1e-7)); detection d takes its same-class label of highest IoU >= 0.5 - among labels
 *  of EQUAL IoU the LOWER label index (numpy leaves that order unspecified) - and is correct at threshold t when that IoU >= IOUV[t]
 *  (fp32 values of torch.linspace(0.5, 0.95, 10)) and no earlier row took the same label with an IoU >= IOUV[t].  A NaN IoU and a class
 *  mismatch never match.  No cap on labels per image.  One launch, one workgroup per image; nothing is allocated, set or synchronised,
 *  so the call can be captured.
 *  TAMTR_EINVAL: a NULL operand (lab_cls / lab_box may be NULL only when M == 0), B < 1, nq < 1, nd < 5, M < 0, dtype not F32 / BF16.
 *  TAMTR_EUNSUP: nq > 512. */
int tamtr_val_postprocess_match(const void* preds, int dtype, int B, int nq, int nd, float imgsz, float conf, float iou, int single_cls,
                                float max_wh, const float* lab_cls, const float* lab_box, const int32_t* lab_off, int M, const float* scale,
                                float* predn, uint8_t* correct, int32_t* counts, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Validator confusion matrix.  Replaces the per-image ConfusionMatrix.process_batch (ultralytics/utils/metrics.py:833-877) as
 * RTDETRValidator.update_metrics calls it (ultralytics/models/rtdetrworld/val.py:141-165).  Reads the outputs of
 * tamtr_val_postprocess_match on the device and the same grouped labels:
 *      predn   f32 [B, nq, 6]   as tamtr_val_postprocess_match leaves it: x1 y1 x2 y2 (original-image pixels), score, cls
 *      counts  i32 [B]          rows of predn that are detections (read on the device; clamped to 0 .. nq)
 *      lab_cls, lab_box, lab_off, M, scale: as for tamtr_val_postprocess_match (only scale[b][2..3] = fp32(w_orig), fp32(h_orig) are used)
 *      matrix  i32 [(nc + 1) * (nc + 1)]   row = predicted, column = true, index nc = background.  ADDED TO in place: the caller zeroes
 *                               it once per run and the accumulation over images, batches and launches stays on the device
 *  The rule, per image with npr = counts[b] detections and nl labels (exact integer equality with engine.ConfusionMatrix on CPU fp32
 *  tensors).  Label boxes: xywh -> xyxy on the normalised values, then x *= fp32(w_orig), y *= fp32(h_orig).  Classes are truncated
 *  towards zero as `.int()` does; a label or a detection whose class is outside [0, nc) (or NaN) is removed first and counted nowhere
 *  (the reference would index out of range).  Under single_cls the classes of predn are already 0; label classes are left as they are.
 *   1. npr == 0: every label adds matrix[nc, gc] += 1.
 *   2. npr > 0 and nl == 0: the matrix is NOT touched - the reference calls process_batch only inside `if nl:`, so detections on an image
 *      without labels are not counted as false positives (kept on purpose).
 *   3. otherwise the detections with score > cm_conf (fp32) take part.  IoU = engine.box_iou(labels, dets) =
 *      inter / (((area_l + area_d) - inter) + fp32(1e-7)), class-agnostic; a pair is a candidate when iou > iou_thres (strict, fp32; a NaN
 *      IoU never qualifies); L(d) = the candidate label of highest IoU of detection d; D(l) = among the detections with L(d) == l the one
 *      of highest IoU.  Among equal IoUs the LOWER label index wins in L and the LOWER detection row wins in D (the reference's
 *      argsort()[::-1] + np.unique passes leave that order unspecified).
 *   4. a label with a D(l) adds matrix[cls(D(l)), gc(l)] += 1; every other label adds matrix[nc, gc(l)] += 1.
 *   5. only if the image has at least one matched pair, every confidence-passing detection that is nobody's D(l) adds
 *      matrix[cls(d), nc] += 1 (the reference's `if n:`): an image whose detections all miss contributes no false positives (kept on
 *      purpose).
 *  cm_conf and iou_thres are compared as given, in fp32.  No cap on labels per image.  One launch, one workgroup per image, integer
 *  atomics only (the result does not depend on order); nothing is allocated, set or synchronised, so the call can be captured.
 *  TAMTR_EINVAL: a NULL operand (lab_cls / lab_box may be NULL only when M == 0), B < 1, nq < 1, nc < 1, M < 0, iou_thres < 0 or NaN.
 *  TAMTR_EUNSUP: nq > 512. */
int tamtr_val_confusion(const float* predn, const int32_t* counts, int B, int nq, int nc, const float* lab_cls, const float* lab_box,
                        const int32_t* lab_off, int M, const float* scale, float cm_conf, float iou_thres, int32_t* matrix, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * The validator's AP per class and IoU threshold and its precision / recall / PR curves in one launch.  Replaces compute_ap and the
 * per-class loop of ap_per_class (ultralytics/utils/metrics.py:999-1029,1073-1127) on rows that never leave the device.
 *      conf     f32 [N]        scores of all rows of the run, SORTED by class ascending, then score descending, then original order
 *      correct  u8  [N, 10]    the rows' hits per IoU threshold, in the same order
 *      seg_off  i32 [nc + 1]   rows seg_off[c] .. seg_off[c + 1] are class c's (read on the device, clamped to 0 .. N); rows before
 *                              seg_off[0] and after seg_off[nc] (dead rows) belong to no class
 *      lab_cls  f32 [M]        the run's label classes, in any order (NULL only when M == 0)
 *      px f64 [1000], grid f64 [101]   numpy's linspace(0, 1, 1000) and linspace(0, 1, 101), uploaded (not recomputed: i / 999.0 has
 *                              other bits)
 *      tpc_scratch i32 [10, N], env_scratch f64 [10, N]    scratch, contents undefined before and after
 *      ap f64 [nc, 10]; p_curve, r_curve, pr_curve f64 [nc, 1000]; n_gt, n_pred i32 [nc]    dense over [0, nc), fully written
 *  The rule is engine.ap_per_class(stable=True, curves=True), all in fp64, one rounding per operation.  n_gt[c] = the labels with
 *  float(c) == class (labels outside [0, nc) are counted nowhere; the host rule would give them a zero row of their own);
 *  n_pred[c] = k = seg_off[c + 1] - seg_off[c].  With n = n_gt[c], rows i = 0 .. k - 1 and threshold t: tpc[i] = inclusive count of
 *  correct[., t]; recall = tpc / (n + 1e-16); precision = tpc / (i + 1).  A class with n == 0 or k == 0 keeps all-zero rows.
 *   ap        knots (0, 1), the curve, (1, 0); envelope = suffix maximum of precision; y = interp(grid, knot recall, envelope);
 *             ap = h * (sum y - 0.5 * (y[0] + y[100])), h = grid[1] - grid[0], the sum serial over g = 0 .. 100.
 *   r_curve   interp(-px, -conf, recall[:, 0], left = 0); p_curve interp(-px, -conf, precision[:, 0], left = 1); right = the last value.
 *   pr_curve  interp(px, knot recall of threshold 0, its envelope).
 *   interp    numpy's: j = largest index with xp[j] <= x; `left` below xp[0]; fp[last] at or beyond xp[last]; fp[j] when x == xp[j];
 *             else ((fp[j+1] - fp[j]) / (xp[j+1] - xp[j])) * (x - xp[j]) + fp[j] as separate operations; repeated xp use the last of the run.
 *  tpc <= n is assumed (a label is matched at most once per threshold).  One workgroup per (class, threshold), tiles of
 *  tamtr_val_ap_tile() rows with a carry, no cap on a segment's length, no atomics: two runs give the same bits.  Nothing is allocated
 *  or synchronised.
 *  TAMTR_EINVAL: a NULL operand (lab_cls may be NULL only when M == 0), an f64 operand not 8-byte or an f32 / i32 operand not 4-byte
 *  aligned, N < 1, nc < 1, M < 0.  TAMTR_EUNSUP: nc > 2^20 or N > 2^30.  The checks come before any GPU call. */
int tamtr_val_ap_curves(const float* conf, const uint8_t* correct, const int32_t* seg_off, int N, int nc, const float* lab_cls, int M,
                        const double* px, const double* grid, int32_t* tpc_scratch, double* env_scratch, double* ap, double* p_curve,
                        double* r_curve, double* pr_curve, int32_t* n_gt, int32_t* n_pred, void* stream);
int tamtr_val_ap_tile(void); /* rows per tile of the scans above (ops.VAL_AP_TILE) */

/* ---------------------------------------------------------------------------------------------------------------
 * CLIP text tower (frozen ViT-B/32 text encoder), fp32 end to end, forward only.  Replaces `clip.tokenize(...)` followed by
 * `text_model.encode_text(...)` = clip.model.CLIP.encode_text as the reference calls it for every training batch
 * (ultralytics/models/rtdetrworld/train.py:148-150), in set_classes (ultralytics/nn/tasks.py:552-571) and for the validator's vocabulary.
 * The attention of a block runs on tamtr_selfattn_fwd (causal mask_bits, ld = 3 W views into the packed in-projection), its two
 * LayerNorms on tamtr_layernorm_fwd.
 *
 *      tamtr_text_embed: `x = self.token_embedding(text) + self.positional_embedding` (CLIP.encode_text):
 *          x[(i, l), :] = tok[ids[i, l], :] + pos[l, :]
 *      ids i32 [n, L]; tok f32 [V, W]; pos f32 [>= L, W]; x f32 [n * L, W].  W % 4 == 0, tok / pos / x 16-byte aligned.  An id outside
 *      [0, V) is never used as an index: its output row is NaN (the Python wrapper refuses such ids before the launch).
 */
int tamtr_text_embed(const int32_t* ids, const float* tok, const float* pos, float* x, long long n, int L, int W, int V, void* stream);

/*      tamtr_linear_f32: the four dense layers of a residual block (nn.MultiheadAttention's packed in-projection and out_proj, mlp.c_fc +
 *      QuickGELU, mlp.c_proj; CLIP's ResidualAttentionBlock.forward):
 *          Y[M,N] = epi( X[M,K] @ W[N,K]^T + bias[N] )      fp32 in and out, fp32 accumulation on v_mfma_f32_32x32x2_f32
 *      epi: 0 none; 1 QuickGELU y * sigmoid(1.702 y); 2 residual add of `residual` f32 [M,N], which may be Y itself (`x = x + ...`).
 *      X f32 [M,K], W f32 [N,K] (nn.Linear layout), both row-major and 16-byte aligned; bias f32 [N] or NULL; residual NULL unless epi == 2.
 *      Requires K % 32 == 0, N % 64 == 0 (TAMTR_EUNSUP otherwise); any M >= 1: the row tail of the last tile is masked inside the kernel,
 *      rows >= M of Y are not touched.  LDS-staged 64 x 64 x 32 tiles, no split-K, no atomics: every element is one ordered sum, the same
 *      bits on every run.
 */
int tamtr_linear_f32(const float* X, const float* W, const float* bias, const float* residual, float* Y, int M, int N, int K, int epi,
                     void* stream);

/*      tamtr_text_pool_project: `x = self.ln_final(x); x = x[arange(n), text.argmax(dim=-1)] @ self.text_projection` (CLIP.encode_text)
 *      and, with norm != 0, `txt_feats / txt_feats.norm(p=2, dim=-1, keepdim=True)` (train.py:150), one workgroup per prompt:
 *          r = first argmax_l ids[i, l];  out[i, :] = LayerNorm(x[(i, r), :]; gamma, beta, eps) @ proj   ( / its L2 norm, no eps )
 *      x f32 [n * L, W]; ids i32 [n, L]; gamma, beta f32 [W]; proj f32 [W, E]; out f32 [n, E].  W <= 1024, E <= 1024.
 */
int tamtr_text_pool_project(const float* x, const int32_t* ids, const float* gamma, const float* beta, const float* proj, float* out, int n,
                            int L, int W, int E, float eps, int norm, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * ByteTrack multi-object tracking.  Replaces BYTETracker.update, ultralytics/trackers/byte_tracker.py:238-351, with its Kalman filter
 * (trackers/utils/kalman_filter.py:33-180: initiate, multi_predict, project, update) and its association (trackers/utils/matching.py:20-126:
 * linear_assignment over lap.lapjv(extend_cost=True, cost_limit=thresh), iou_distance, fuse_score), as trackers/track.py:40-53 calls it
 * once per frame on the host.  (New symbols only; the ABI version stays 36.)
 *
 *  out f32 [B, nq, 6], counts i32 [B]: the output of tamtr_detect_postprocess; the B frames are consumed in order inside one launch.
 *  tracks f32 [B, nq, 8]: x1 y1 x2 y2 id score cls idx per activated track in state Tracked, the box from the filter mean, idx the row
 *  of `out` the track was last matched to; rows after tcounts[b] are zero.  A frame with counts[b] <= 0 does not reach the tracker:
 *  the frame counter does not advance and nothing ages (track.py:46-47).
 *  The tracker's state is a table of T slots that the caller owns and the kernel updates in place:
 *      mean f64 [T, 8], cov f64 [T, 8, 8], sc f32 [T, 2] (score, cls), hdr i32 [8] (frame_id, next_id, live slots, overflow, 0...),
 *      meta i32 [T, 8] (state, is_activated, track_id, frame_id, start_frame, tracklet_len, idx, flags)
 *  with state 0 free / 1 Tracked / 2 Lost / 3 Removed but still listed for one update, and flags 1 = mean is the untouched fp32
 *  measurement, 2 = id is in the reference's removed list (csrc/track.hip states both).  A fresh table is all zero except
 *  hdr[1] = 1 (ids start at 1).  A new track that finds no free slot is not created and is counted in hdr[3]; nothing is written
 *  outside the T slots.
 *  Arithmetic: the filter in fp64 as numpy, the costs in fp32 in the reference's operation order (the object is compiled with
 *  -ffp-contract=off), scores compared in fp32; each assignment is the optimum lap.lapjv returns (the partial matching minimising
 *  sum(c_ij - thresh)), found by lsap.hip's solver with one shared `unmatched` column - the reference's matching wherever it is unique.
 *  workspace: tamtr_bytetrack_workspace_bytes(T, nq) bytes of device memory, 16-byte aligned, contents irrelevant (0 = unsupported).
 *  One launch, one workgroup; nothing is allocated, set or synchronised, so the call can be captured.
 *  TAMTR_EINVAL: a NULL operand, B < 1, nq < 1, T < 1, a workspace that is too small.  TAMTR_EUNSUP: T and nq whose solver state
 *  (about 12 T + 30 nq bytes) exceeds 64 KiB of LDS.  The checks come before any GPU call. */
int tamtr_bytetrack_update(const float* out, const int32_t* counts, int B, int nq, double* mean, double* cov, int32_t* meta, float* sc,
                           int32_t* hdr, int T, float track_high_thresh, float track_low_thresh, float new_track_thresh,
                           double match_thresh, int max_time_lost, float* tracks, int32_t* tcounts, void* workspace, int workspace_bytes,
                           void* stream);
int tamtr_bytetrack_workspace_bytes(int T, int nq);

/*      tamtr_botsort_update: BOTSORT.update, ultralytics/trackers/bot_sort.py (with STrack.multi_gmc, byte_tracker.py:81-97, and
 *      KalmanFilterXYWH, utils/kalman_filter.py:222-368), for the B frames of a batch: the launch, the table, the workspace
 *      (tamtr_bytetrack_workspace_bytes) and the error codes of tamtr_bytetrack_update, with the filter state (x, y, w, h and their
 *      velocities), mean[6] = mean[7] = 0 before a track that is not Tracked is predicted, and the frame's warp applied to every pool
 *      and every unconfirmed track between the prediction and the first association (csrc/track.hip states all three).
 *      warps f64 [B, 2, 3], row-major, in the pixels of `out`, on the device, 8-byte aligned (else TAMTR_EINVAL); NULL = the identity
 *      for every frame.  The warp of a frame with counts[b] <= 0 is not applied.  This entry is the tracker with with_reid off - as
 *      the reference runs it, which builds no embeddings: the costs are ByteTrack's, and proximity_thresh and appearance_thresh are
 *      arguments of tamtr_botsort_reid_update below only.  A table written by one of
 *      the two trackers must not be handed to the other: the means differ in meaning.  (New symbol only; the ABI version stays 36.) */
int tamtr_botsort_update(const float* out, const int32_t* counts, const double* warps, int B, int nq, double* mean, double* cov,
                         int32_t* meta, float* sc, int32_t* hdr, int T, float track_high_thresh, float track_low_thresh,
                         float new_track_thresh, double match_thresh, int max_time_lost, float* tracks, int32_t* tcounts, void* workspace,
                         int workspace_bytes, void* stream);

/*      tamtr_botsort_reid_update: BOTSORT.update with with_reid on - the appearance half of the rule, which the reference writes out
 *      (BOTrack.update_features bot_sort.py:55-64, BOTSORT.init_track :166-174, BOTSORT.get_dists :176-190,
 *      matching.embedding_distance utils/matching.py:84-105) and never runs for want of an encoder.  tamtr_botsort_update's operands,
 *      table, outputs and launch, plus
 *      feat  f32 [B, nq, D]  one feature row per row of `out` (tamtr_reid_rows writes them; rows after counts[b] are not read),
 *      tfeat f32 [T, D]      the table's smooth_feat per slot, updated in place; a fresh table needs no fill (a new track copies
 *                            its detection's row),
 *      proximity_thresh (compared in fp32 with the raw IoU distance) and appearance_thresh (compared in fp64 with the halved cosine
 *      distance): in the first association and in the unconfirmed tracks' a pair whose IoU distance is not above proximity_thresh
 *      costs min(fused IoU distance, e), e = max(0, cosine distance) / 2 set to 1 where it is above appearance_thresh; matched tracks
 *      smooth their row with alpha = 0.9 and renormalise it (csrc/track.hip states the arithmetic and the summation orders).  With
 *      appearance_thresh < 0 no embedding can act and rows and table are those of tamtr_botsort_update, bit for bit.
 *      workspace: tamtr_botsort_reid_workspace_bytes(T, nq) bytes (the cost matrix is fp64 here), 8-byte aligned.
 *      TAMTR_EINVAL: as tamtr_botsort_update, a NULL feat or tfeat, D < 1, a misaligned or too small workspace.  TAMTR_EUNSUP:
 *      D > 1024, and as tamtr_bytetrack_update.  The checks come before any GPU call; one launch, nothing allocated, set or
 *      synchronised.  (New symbols only; the ABI version stays 36.) */
int tamtr_botsort_reid_update(const float* out, const int32_t* counts, const double* warps, const float* feat, int B, int nq,
                              double* mean, double* cov, int32_t* meta, float* sc, int32_t* hdr, float* tfeat, int D, int T,
                              float track_high_thresh, float track_low_thresh, float new_track_thresh, double match_thresh,
                              int max_time_lost, float proximity_thresh, double appearance_thresh, float* tracks, int32_t* tcounts,
                              void* workspace, int workspace_bytes, void* stream);
int tamtr_botsort_reid_workspace_bytes(int T, int nq);

/*      tamtr_reid_rows: the feature rows tamtr_botsort_reid_update reads, gathered from a per-query embedding (e.g. the decoder's
 *      hidden state that goes into the score head) by the `keep` of tamtr_detect_postprocess: feat[b, j, :] = embed[b, keep[b, j], :]
 *      widened to fp32 and divided by its norm twice, as BOTrack.__init__ -> update_features does to a detection's feature
 *      (bot_sort.py:50-64: feat /= |feat|, then smooth_feat, the same array, /= |smooth_feat|), for j < counts[b]; zero rows after.
 *      embed (T) [B, nqm, D] (dtype TAMTR_F32 or TAMTR_BF16), keep i32 [B, nq], counts i32 [B], feat f32 [B, nq, D].  A keep index
 *      outside [0, nqm) gives a zero row; a row of zero norm is outside the contract.  One wavefront per row, 16-byte loads where
 *      D % 4 == 0 and the bases are aligned; csrc/track.hip states the order of the sums.
 *      TAMTR_EINVAL: a NULL operand, B, nqm, nq or D < 1.  TAMTR_EUNSUP: D > 1024, another dtype.  One launch, checks first. */
int tamtr_reid_rows(const void* embed, int dtype, const int32_t* keep, const int32_t* counts, int B, int nqm, int nq, int D, float* feat,
                    void* stream);

/*      tamtr_gmc_estimate: the warps tamtr_botsort_update reads, estimated from the frames of the batch on the device.  It stands where
 *      the reference runs OpenCV on the host (trackers/utils/gmc.py:247-302, applySparseOptFlow); the rule is the project's own and is
 *      written out in csrc/gmc.hip (grey + pyramid, grid keypoints, pyramidal Lucas-Kanade, 512-hypothesis similarity fit).
 *      frames u8 [B, H, W, 3] RGB, the network input as uploaded; H, W multiples of 8 and at least 64 (else TAMTR_EINVAL)
 *      counts i32 [B]        the detections per frame: a frame with counts[b] <= 0 gets the identity and never becomes "previous"
 *      scale  f64 [B, 2]     (sx, sy) = (w0 / W, h0 / H): network pixels -> the original pixels the tracker's states live in
 *      st_pyr u8 [tamtr_gmc_state_bytes(H, W)], st_kp i32 [1024], st_hdr i32 [4]   the persistent state: pyramid and keypoint slots of
 *                            the last frame that reached the tracker, st_hdr[0] = valid; updated in place; st_hdr all zero = fresh
 *      warps  f64 [B, 2, 3]  out, original pixels, warp b maps the paired earlier frame's coordinates to frame b's
 *      stats  i32 [B, 4]     out: keypoints, tracked, inliers, used
 *      workspace: tamtr_gmc_workspace_bytes(B, H, W) bytes, 16-byte aligned, contents irrelevant.  tamtr_gmc_workspace_offset(B, H, W, i)
 *      is the byte offset of section i (csrc/gmc.hip lists them: pyramids, corner response, tile maxima, keypoint slots, point pairs,
 *      status, fit record, pairing), so that a test can read and prescribe every stage; `stages` is a mask of the launches to run
 *      (1 pyramid + corner response, 2 cells, 4 LK, 8 fit + state copy; 15 = all, the only value outside tests).
 *      At most four launches on `stream`; nothing is allocated, set or synchronised.  Every check comes before any GPU call.
 *      (New symbols only; the ABI version stays 36.) */
int tamtr_gmc_workspace_bytes(int B, int H, int W);      /* -1: H, W or B outside what is built, or more than 2^31 - 1 bytes */
int tamtr_gmc_workspace_offset(int B, int H, int W, int which);
int tamtr_gmc_state_bytes(int H, int W);
int tamtr_gmc_estimate(const uint8_t* frames, const int32_t* counts, const double* scale, int B, int H, int W, uint8_t* st_pyr,
                       int32_t* st_kp, int32_t* st_hdr, double* warps, int32_t* stats, void* workspace, int workspace_bytes,
                       int stages, void* stream);

/*      Several streams at once: one tracker per stream, one launch.  Replaces trackers/track.py:33-53, where on_predict_start builds
 *      predictor.trackers[i] for i in range(bs) and on_predict_postprocess_end walks the images of the batch on the host, image i to
 *      tracker i.  A batch holds B = F * S images, frame-major: image f * S + s is the f-th frame of stream s (F = 1 is the live case).
 *      The tables are stacked: mean f64 [S, T, 8], cov f64 [S, T, 8, 8], meta i32 [S, T, 8], sc f32 [S, T, 2], hdr i32 [S, 8]
 *      [, tfeat f32 [S, T, D]]; out, counts, warps, feat, tracks and tcounts keep their shapes over the B images.  Workgroup s owns
 *      tracker s and walks its images in order; the workgroups share nothing, so stream s gets what the single-tracker entry point
 *      computes on its images and its slice of the tables, bit for bit - the single-tracker entry points are these with S = 1.  A stream
 *      without a frame at some position (ended, or a dropped frame) keeps its image with counts = 0: it does not reach the tracker.
 *      workspace: tamtr_bytetrack_streams_workspace_bytes(S, T, nq) (tamtr_botsort_reid_streams_workspace_bytes for the ReID entry)
 *      bytes, 16-byte aligned: S times the single-tracker size rounded up to 16 (0 = unsupported).
 *      TAMTR_EINVAL: as the single-tracker entry, and S < 1 or B % S != 0.  TAMTR_EUNSUP: as there (LDS is per workgroup).
 *      (New symbols only: no existing signature changed, the ABI version stays 36.) */
int tamtr_bytetrack_update_streams(const float* out, const int32_t* counts, int B, int S, int nq, double* mean, double* cov, int32_t* meta,
                                   float* sc, int32_t* hdr, int T, float track_high_thresh, float track_low_thresh, float new_track_thresh,
                                   double match_thresh, int max_time_lost, float* tracks, int32_t* tcounts, void* workspace,
                                   int workspace_bytes, void* stream);
int tamtr_bytetrack_streams_workspace_bytes(int S, int T, int nq);
int tamtr_botsort_update_streams(const float* out, const int32_t* counts, const double* warps, int B, int S, int nq, double* mean, double* cov,
                                 int32_t* meta, float* sc, int32_t* hdr, int T, float track_high_thresh, float track_low_thresh,
                                 float new_track_thresh, double match_thresh, int max_time_lost, float* tracks, int32_t* tcounts,
                                 void* workspace, int workspace_bytes, void* stream);
int tamtr_botsort_reid_update_streams(const float* out, const int32_t* counts, const double* warps, const float* feat, int B, int S, int nq,
                                      double* mean, double* cov, int32_t* meta, float* sc, int32_t* hdr, float* tfeat, int D, int T,
                                      float track_high_thresh, float track_low_thresh, float new_track_thresh, double match_thresh,
                                      int max_time_lost, float proximity_thresh, double appearance_thresh, float* tracks,
                                      int32_t* tcounts, void* workspace, int workspace_bytes, void* stream);
int tamtr_botsort_reid_streams_workspace_bytes(int S, int T, int nq);

/*      tamtr_gmc_estimate_streams: tamtr_gmc_estimate for the same frame-major batch of S streams, with the state stacked: st_pyr u8
 *      [S, tamtr_gmc_state_bytes(H, W)], st_kp i32 [S, 1024], st_hdr i32 [S, 4].  Frame i is paired with the nearest earlier frame
 *      i - k S of its stream whose count is positive, else with stream i % S's state if that is valid, else with nothing; afterwards
 *      stream s's state holds its last frame with a positive count and is untouched if it had none.  The same four launches for the
 *      whole batch, the same workspace (tamtr_gmc_workspace_bytes(B, H, W)); S = 1 is tamtr_gmc_estimate.
 *      TAMTR_EINVAL: as tamtr_gmc_estimate, and S < 1 or B % S != 0.  (New symbol only; the ABI version stays 36.) */
int tamtr_gmc_estimate_streams(const uint8_t* frames, const int32_t* counts, const double* scale, int B, int S, int H, int W, uint8_t* st_pyr,
                               int32_t* st_kp, int32_t* st_hdr, double* warps, int32_t* stats, void* workspace, int workspace_bytes,
                               int stages, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * COCO-protocol bbox evaluation (AP / AR by object size) on the device.  Replaces the step the reference leaves to pycocotools:
 * valTAMTR.py:15 (save_json=True "if you need to cal coco metrice"), dataset/yolo2coco.py (the annotation file for it) and
 * requirements.txt:44 (pycocotools, "COCO mAP").  The rule is written out in csrc/cocoeval.hip and stated by engine.coco_evaluate.
 *
 * tamtr_val_coco_match: the per-image matching of a whole batch, one launch, one workgroup per image.
 *      predn f32 [B, nq, 6], counts i32 [B]                 outputs of tamtr_val_postprocess_match (rows in descending score order)
 *      lab_cls f32 [M], lab_box f32 [M, 4], lab_off i32 [B + 1], scale f32 [B, 4]     the labels as tamtr_val_confusion reads them
 *      thresholds f64 [10]                                  numpy's linspace(0.5, 0.95, 10)
 *      max_det                                              the last entry of max_dets: rows of rank >= max_det take part in nothing
 *      bits i32 [B, nq, 4]   per row and size range (all, small, medium, large): bit t = matched at threshold t, bit 16 + t = ignored
 *      rank i32 [B, nq]      the row's rank among the image's rows of its class that take part; -1 for a row that takes part in
 *                            nothing (row >= counts[b], class outside [0, nc), NaN score)
 *      npig i32 [nc, 4]      ADDED TO: the non-ignored ground truths per class and range (integer atomics, order-free)
 *      workspace             tamtr_val_coco_workspace_bytes(B, nq, M) bytes, 16-byte aligned, contents irrelevant: the label table of an
 *                            image with more than 512 labels (no cap on labels per image)
 *  Nothing is allocated, set or synchronised.  TAMTR_EINVAL: a NULL operand (lab_cls / lab_box may be NULL only when M == 0), B < 1,
 *  nq < 1, nc < 1, M < 0, max_det < 1, a misaligned operand, a workspace that is too small.  TAMTR_EUNSUP: nq > 512.
 *
 * tamtr_val_coco_accumulate: the accumulation of a whole run, one launch, one workgroup per (class, range, cut, threshold).
 *      bits i32 [N, 4], rank i32 [N]     the rows of the run sorted by class, then score descending, then original order
 *      seg_off i32 [nc + 1]              rows of class k are seg_off[k] .. seg_off[k + 1]
 *      npig i32 [nc, 4], max_dets i32 [n_max_dets] (ascending, 1 .. 4 entries), grid f64 [101] = numpy's linspace(0, 1, 101)
 *      precision f64 [10, 101, nc, 4, n_max_dets]; recall, ap_tkam f64 [10, nc, 4, n_max_dets]     fully written
 *  ap_tkam = the mean of precision over the 101 grid values, summed serially in grid order; -1 stays -1.  No atomics and no
 *  floating-point reduction whose order could vary: two runs give the same bits.
 *  TAMTR_EINVAL: a NULL or misaligned operand, N < 1, nc < 1, n_max_dets outside 1 .. 4.  TAMTR_EUNSUP: nc > 2^16 or N > 2^30. */
int tamtr_val_coco_match(const float* predn, const int32_t* counts, int B, int nq, int nc, const float* lab_cls, const float* lab_box,
                         const int32_t* lab_off, int M, const float* scale, const double* thresholds, int max_det, int32_t* bits,
                         int32_t* rank, int32_t* npig, void* workspace, int workspace_bytes, void* stream);
int tamtr_val_coco_workspace_bytes(int B, int nq, int M); /* 0 = unsupported */
int tamtr_val_coco_accumulate(const int32_t* bits, const int32_t* rank, const int32_t* seg_off, int N, int nc, const int32_t* npig,
                              const int32_t* max_dets, int n_max_dets, const double* grid, double* precision, double* recall,
                              double* ap_tkam, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * MOT evaluation on the device: CLEAR-MOT (MOTA, MOTP, FP, FN, IDSW, Frag, MT / PT / ML) and identity (IDF1, IDP, IDR) counts of the
 * tracker's rows against ground truth, per class (TrackEval's CLEAR and Identity definitions).  The rule is written out in
 * csrc/mot.hip and stated by engine.mot_evaluate.
 *
 * State, owned by the caller, all zero when fresh, updated in place (G = G_cap gt identities, T = T_cap track ids):
 *      gstate i32 [G, 8]     last-matched track id + 1, frames present, frames matched, runs, last matched frame, class + 1, 0, 0
 *      counts i32 [nc, 16]   TP FN FP IDSW gt_dets trk_dets Frag MT PT ML IDTP gt_ids drop_region drop_distractor 0 0 (run totals)
 *      iou_sum f64 [nc]      pair i32 [G, T]      hdr i32 [8] (frame counter, gt ids beyond G, track ids beyond T, rows beyond ng / nq)
 *
 * tamtr_mot_update: steps 1 to 4 of the rule for the B frames of a batch, in order, one launch, one workgroup.
 *      tracks f32 [B, nq, 8], tcounts i32 [B]    exactly as tamtr_bytetrack_update leaves them (id in column 4, class in column 6)
 *      gt f32 [B, ng, 7], gcounts i32 [B]        x1 y1 x2 y2 id cls kind; the id of a kind-0 row is its dense row in [0, G)
 *  An id outside its table or a count beyond ng / nq is counted in hdr and the rows are left out; nothing is written past a table.
 *  The CLEAR counts and iou_sum (an fp64 atomic add: its last bits depend on the order) go straight into the run totals.
 * tamtr_mot_end_sequence: one launch, one workgroup per class: MT / PT / ML / Frag / gt_ids and the identity assignment (IDTP) of the
 *  sequence are added to counts; gstate, the used rows of pair and the frame counter are cleared.  G_used: the dense rows handed out.
 * workspace: tamtr_mot_workspace_bytes(nq, ng, nc, G_cap, T_cap) bytes of device memory for either call, 16-byte aligned, contents
 *  irrelevant (0 = unsupported).  Nothing is allocated, set or synchronised.
 * TAMTR_EINVAL: a NULL or misaligned operand, a size < 1, iou_thr <= 0, a workspace that is too small.  TAMTR_EUNSUP: ng and nq whose
 *  solver state (about 12 ng + 30 nq bytes) exceeds 60 KiB of LDS, G_cap * T_cap > 2^31 - 1, an id range fp32 cannot carry. */
int tamtr_mot_update(const float* tracks, const int32_t* tcounts, const float* gt, const int32_t* gcounts, int B, int nq, int ng, int nc,
                     double iou_thr, int32_t* gstate, int32_t* counts, double* iou_sum, int32_t* pair, int32_t* hdr, int G_cap, int T_cap,
                     void* workspace, int workspace_bytes, void* stream);
int tamtr_mot_end_sequence(int nc, int32_t* gstate, int32_t* counts, int32_t* pair, int32_t* hdr, int G_cap, int T_cap, int G_used,
                           void* workspace, int workspace_bytes, void* stream);
int tamtr_mot_workspace_bytes(int nq, int ng, int nc, int G_cap, int T_cap); /* 0 = unsupported */

/* ---------------------------------------------------------------------------------------------------------------
 * HOTA on the device, next to the MOT evaluation: the counts behind HOTA, DetA, AssA, DetRe / DetPr, AssRe / AssPr and LocA at the 19
 * localisation thresholds, per class (TrackEval's HOTA.eval_sequence).  The rule is written out in csrc/hota.hip and stated by
 * engine.hota_evaluate.
 *
 * state: a HOST array of 12 device pointers, all zero when fresh, updated in place; caps: a HOST array of the 5 capacities G (gt
 * identities), T (track ids), P (pair slots), L (log entries), F (frames of a sequence).  In order:
 *      gstate i32 [G, 2]  frames present, class + 1          tcount i32 [nc, T]  frames a track identity is present in
 *      pkey i64 [P]  ((gt row << 32) | track id) + 1, 0 free ppot f64 [P]  the pair's pot      phist i32 [P, 20]  its matches by level
 *      fidx i32 [F, 4]  first log entry, entries, n, m       log i32 [L, 4]  per positive pair: S (f64), slot (i32), row, column (u16)
 *      dets i32 [nc, 2]  gt_dets, trk_dets                   tp_lvl i32 [nc, 20]      loc_lvl f64 [nc, 20]      ass f64 [3, nc, 19]
 *      hdr i32 [16]  frames logged, log entries used, then what was left out: gt ids beyond G, track ids beyond T, rows beyond ng / nq,
 *                    pairs beyond L, frames beyond F, pairs without a slot, 0 ...
 *  A pair matched at level k (the number of thresholds its IoU passed) is a TP at every threshold a < k: TP[c, a] is the sum of
 *  tp_lvl[c, k] over k > a, loc_sum likewise.  dets, tp_lvl, loc_lvl and ass are run totals; the rest belongs to the open sequence.
 *
 * tamtr_hota_update: steps 1 and 2 of the MOT rule, then pass 1 (presence counts, pot) and the log, for the B frames of a batch, in
 *  order, one launch, one workgroup.  tracks / tcounts / gt / gcounts as tamtr_mot_update takes them; eps = DBL_EPSILON.
 *  Whatever exceeds a capacity is counted in hdr and left out; nothing is written past a table.
 * tamtr_hota_end_sequence: pass 2 and the reduction in three launches: `workgroups` workgroups stride over the logged frames and match
 *  each (scores gas * S), bumping the level bins; one thread per pair slot adds the pair's terms to ass and clears the slot; the
 *  sequence's gstate, tcount and counters are cleared.  alpha: HOST pointer to the 19 thresholds, np.arange(0.05, 0.99, 0.05) as made.
 * workspace: tamtr_hota_workspace_bytes(nq, ng, workgroups) bytes of device memory for either call (update: workgroups is irrelevant),
 *  16-byte aligned, contents irrelevant (0 = unsupported).  Nothing is allocated, set or synchronised.
 * TAMTR_EINVAL: a NULL or misaligned operand, a size or capacity < 1, iou_thr or eps <= 0, a workspace that is too small.
 *  TAMTR_EUNSUP: ng and nq whose solver state exceeds 60 KiB of LDS or 65535, workgroups > 1024, nc * T or 20 P > 2^31 - 1, an id range
 *  fp32 cannot carry. */
int tamtr_hota_update(const float* tracks, const int32_t* tcounts, const float* gt, const int32_t* gcounts, int B, int nq, int ng, int nc,
                      double iou_thr, double eps, void* const* state, const int* caps, void* workspace, int workspace_bytes, void* stream);
int tamtr_hota_end_sequence(const double* alpha, double eps, int nc, int nq, int ng, int workgroups, void* const* state, const int* caps,
                            void* workspace, int workspace_bytes, void* stream);
int tamtr_hota_workspace_bytes(int nq, int ng, int workgroups); /* 0 = unsupported */

/*      Several streams at once: one evaluator state per stream, scored next to tamtr_*_update_streams on the same frame-major batch
 *      (image f * S + s is the f-th frame of stream s, B = F * S).  Every state tensor of either evaluator gains a leading S (MOT: gstate
 *      [S, G, 8], counts [S, nc, 16], iou_sum [S, nc], pair [S, G, T], hdr [S, 8]; HOTA: all twelve likewise, the state array still holds
 *      12 pointers), and slice s is a valid single-evaluator state: the single entries accept state[k][s] as it is.
 *      tamtr_mot_update_streams / tamtr_hota_update_streams: one launch, grid = S; workgroup s walks images s, s + S, ... in order and
 *       touches only slice s of the state and of the workspace, the run totals included: no atomic is shared between streams, so stream s
 *       gets what the single entry computes on its images.  active i32 [B] on the device, NULL = every image counts: an image whose
 *       word is 0 is no frame of its stream - it advances no frame counter, logs and counts nothing, and its rows are not read (a stream
 *       that has ended keeps its place in the batch so, and a stream without ground truth stays unscored).
 *      tamtr_mot_end_streams: one launch, grid (nc, S).  ending i32 [S] on the device, NULL = every stream ends: the workgroups of a
 *       stream whose word is 0 return at once and leave slice s untouched; the others do what tamtr_mot_end_sequence does, on slice s,
 *       with gt_used[s] (i32 [S] on the device) as its G_used.
 *      tamtr_hota_end_streams: the three launches of tamtr_hota_end_sequence with the stream as the grid's second dimension and the same
 *       `ending` mask; `workgroups` is per stream (ops: min(64, 1024 / S), at least 1), each with its own workspace slice.
 *      workspace: tamtr_mot_streams_workspace_bytes(S, nq, ng, nc, G_cap, T_cap) / tamtr_hota_streams_workspace_bytes(S, nq, ng,
 *       workgroups) bytes, 16-byte aligned: S times the single size rounded up to 16; 0 = a size the single entry does not support, or a
 *       total beyond 2^31 - 1 bytes.  LDS use is per workgroup and unchanged.
 *      TAMTR_EINVAL / TAMTR_EUNSUP: as the single entries, and TAMTR_EINVAL for S < 1, B % S != 0 or a NULL gt_used; TAMTR_EUNSUP for
 *       S > 65535.  Every check comes before any GPU call; nothing is allocated, set or synchronised.  The single entries are these
 *       with S = 1 and NULL masks.  (New symbols only: no existing signature changed, the ABI version stays 36.) */
int tamtr_mot_update_streams(const float* tracks, const int32_t* tcounts, const float* gt, const int32_t* gcounts, int B, int S, int nq, int ng,
                             int nc, double iou_thr, const int32_t* active, int32_t* gstate, int32_t* counts, double* iou_sum, int32_t* pair,
                             int32_t* hdr, int G_cap, int T_cap, void* workspace, int workspace_bytes, void* stream);
int tamtr_mot_end_streams(int nc, int S, const int32_t* ending, const int32_t* gt_used, int32_t* gstate, int32_t* counts, int32_t* pair,
                          int32_t* hdr, int G_cap, int T_cap, void* workspace, int workspace_bytes, void* stream);
int tamtr_mot_streams_workspace_bytes(int S, int nq, int ng, int nc, int G_cap, int T_cap); /* 0 = unsupported */
int tamtr_hota_update_streams(const float* tracks, const int32_t* tcounts, const float* gt, const int32_t* gcounts, int B, int S, int nq, int ng,
                              int nc, double iou_thr, double eps, const int32_t* active, void* const* state, const int* caps, void* workspace,
                              int workspace_bytes, void* stream);
int tamtr_hota_end_streams(const double* alpha, double eps, int nc, int S, const int32_t* ending, int nq, int ng, int workgroups,
                           void* const* state, const int* caps, void* workspace, int workspace_bytes, void* stream);
int tamtr_hota_streams_workspace_bytes(int S, int nq, int ng, int workgroups); /* 0 = unsupported */

/* ---------------------------------------------------------------------------------------------------------------
 * Track-mAP on the device, next to the MOT evaluation and HOTA: average precision over whole tracks, ranked by mean score and matched
 * to ground-truth tracks by spatio-temporal IoU (TrackEval's TrackMAP for boxes, no area or time ranges; VisDrone-MOT's ranking
 * score).  The rule is written out in csrc/trackmap.hip and stated by engine.track_map_evaluate.
 *
 * state: a HOST array of 10 device pointers, all zero when fresh, updated in place; caps: a HOST array of the 4 capacities G (gt
 * identities), T (track ids), P (pair slots), R (rows of the run's table).  In order:
 *      gstate i32 [G, 2]  frames present, class + 1          garea f64 [G]  the identity's area sum
 *      tframes i32 [nc, T]  frames a track identity is present in      tsum f64 [nc, T, 2]  its area sum, its score sum
 *      pkey i64 [P]  ((gt row << 32) | track id) + 1, 0 free pinter f64 [P]  the pair's intersection sum
 *      rscore f64 [R]  a track's mean score                  rmeta i32 [R, 2]  its class, its bits (bit a = matched at threshold a)
 *      gt_tracks i32 [nc]  ground-truth identities
 *      hdr i32 [16]  run rows used, sequences ended, then what was left out: gt ids beyond G, track ids beyond T, rows beyond ng / nq,
 *                    pairs without a slot, tracks beyond R, 0 ...
 *  rscore, rmeta, gt_tracks and hdr belong to the run; the rest to the open sequence.
 *
 * tamtr_trackmap_update: steps 1 and 2 of the MOT rule, then the area, score and intersection sums, for the B frames of a batch, in
 *  order, one launch, one workgroup: plain fp64 adds in frame order, no floating-point atomics.  tracks / tcounts / gt / gcounts as
 *  tamtr_mot_update takes them; a track's score is column 5 of its row.
 * tamtr_trackmap_end_sequence: six launches: mean scores; the tracks' order per class (score descending, id ascending; a counting
 *  rank against LDS tiles, for any T) with the candidates per track; their offsets; the candidate lists (gt row, IoU); the greedy
 *  matching, one wave per (threshold, class), serial over the tracks; the append to the run's table, and the sequence's state
 *  cleared.  thresholds: HOST pointer to 1 .. 10 fp64 values; eps = DBL_EPSILON.  The run's accumulation is
 *  tamtr_val_coco_accumulate on rmeta's bits (one range, one cut).
 *  Whatever exceeds a capacity is counted in hdr and left out; nothing is written past a table.
 * workspace: tamtr_trackmap_workspace_bytes(nq, ng, nc, G, T, P) bytes of device memory for either call (end_sequence: nq and ng are
 *  irrelevant), 16-byte aligned, contents irrelevant (0 = unsupported).  Nothing is allocated, set or synchronised.
 * TAMTR_EINVAL: a NULL or misaligned operand, a size or capacity < 1, n_thresholds outside 1 .. 10, iou_thr or eps <= 0, a workspace
 *  that is too small.  TAMTR_EUNSUP: ng and nq whose solver state exceeds 60 KiB of LDS or 65535, nc > 4096, G or T > 2^24, P > 2^28,
 *  R > 2^30, a workspace beyond 2^31 - 1 bytes. */
int tamtr_trackmap_update(const float* tracks, const int32_t* tcounts, const float* gt, const int32_t* gcounts, int B, int nq, int ng,
                          int nc, double iou_thr, void* const* state, const int* caps, void* workspace, int workspace_bytes, void* stream);
int tamtr_trackmap_end_sequence(const double* thresholds, int n_thresholds, double eps, int nc, void* const* state, const int* caps,
                                void* workspace, int workspace_bytes, void* stream);
int tamtr_trackmap_workspace_bytes(int nq, int ng, int nc, int G_cap, int T_cap, int P_cap); /* 0 = unsupported */

/* ---------------------------------------------------------------------------------------------------------------
 * Test-time augmentation.  Replaces DetectionModel._predict_augment, ultralytics/nn/tasks.py:272-295, with scale_img
 * (utils/torch_utils.py:316-327) and _descale_pred (tasks.py:286-295), as `augment` reaches them from the predictor and the validator
 * (engine/predictor.py:135, engine/validator.py:109,169).  _clip_augmented (tasks.py:297-306) is anchor-layer specific and has no
 * counterpart for a query decoder.  (New symbols only; the ABI version stays 36.)
 *
 * tamtr_tta_view: scale_img(x.flip(3) if flip else x, ratio, gs) (torch_utils.py:316-327) for a batch in one launch.
 *      x   f32 [B, 3, H, W]    the model input (already / 255)
 *      out f32 [B, 3, Hp, Wp]  the view
 *  The caller computes the sizes in double: content (sh, sw) = (int(H ratio), int(W ratio)), canvas (Hp, Wp) = (ceil(H ratio / gs) gs,
 *  ceil(W ratio / gs) gs).  Inside the content rectangle: torch's bilinear align_corners=False sample of x (of x mirrored left-right
 *  when flip = 1), coordinates in fp32 (csrc/tta.hip states them); outside: 0.447f.  (sh, sw) = (H, W) is a copy, bit for bit.
 *  TAMTR_EINVAL: a NULL operand, B, H, W, sh or sw < 1, Hp < sh, Wp < sw, flip not 0 / 1.  TAMTR_EUNSUP: B or Hp > 65535.
 *
 * tamtr_tta_merge: the views' de-augmented rows concatenated along the query axis (tasks.py:281-284) and merged by the ordinary NMS
 * (models/rtdetrworld/predict.py:34-78), for a batch in one launch, one workgroup per image.
 *      ys      HOST array of V device pointers, each (dtype) [B, nq, 4 + nc]: cx cy w h in 0..1 of the view's canvas, class scores
 *      views   f32 [V, 4]       kx, ky, flip (0 / 1), 0 per view: cx' = cx kx, then 1 - cx' when flip; cy' = cy ky; w' = w kx; h' = h ky
 *      classes i32 [n_classes] or NULL (no class filter)
 *      ym      f32 [B, max_out, 4 + nc]  the first max_out NMS survivors in order: cx' cy' w' h', the source row's scores; zero rows after
 *      src     i32 [B, max_out]  the candidate i = v nq + q a row came from, -1 after counts[b]
 *      counts  i32 [B]           rows written
 *      dropped i32 [B]           survivors that did not fit into max_out rows
 *  Bit-exact in fp32, every operation rounded on its own: score / class / filter / order / NMS as tamtr_detect_postprocess on the
 *  de-augmented candidates (equal scores: ascending i; IoU > iou compared in fp32).  Nothing is written past a table; nothing is
 *  allocated, set or synchronised, so the call can be captured.
 *  TAMTR_EINVAL: a NULL operand or view pointer, V, B, nq or max_out < 1, nd < 5, n_classes < 0, dtype not F32 / BF16.
 *  TAMTR_EUNSUP: V nq > 2048, V > 16, max_out > 512. */
int tamtr_tta_view(const float* x, float* out, int B, int H, int W, int sh, int sw, int Hp, int Wp, int flip, void* stream);
int tamtr_tta_merge(const void* const* ys, int V, int dtype, int B, int nq, int nd, const float* views, float conf, float iou,
                    int single_cls, float max_wh, const int32_t* classes, int n_classes, int max_out, float* ym, int32_t* src,
                    int32_t* counts, int32_t* dropped, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Sliced prediction for large frames.  Replaces nothing of the reference, whose predictor stretches the whole frame to imgsz
 * (LetterBox(scaleFill=True), models/rtdetrworld/predict.py:80-92); it replaces the host loop of sliced inference around a detector:
 * crop overlapping windows, resize each to imgsz, forward, shift the boxes back, merge with the whole-frame view's.  The two rules are
 * stated in tam-tr_amd/slicing.py (views_host, merge_host).  (New symbols only; the ABI version stays 36.)
 *
 * tamtr_slice_views: the windows of ONE original frame as network inputs, in one launch.
 *      src     u8  [h, w, 3]     the original RGB frame on the device
 *      windows HOST i32 [V, 4]   x0 y0 x1 y1 in pixels, 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h (checked here, passed by value)
 *      out     f32 [V, 3, S, S]  out[v] = CHW(float(resize_linear_u8(src[y0:y1, x0:x1], S, S)) * float(1.0 / 255.0))
 *  resize_linear_u8 is tamtr_resize_linear_u8 (tamtr_host.h) bit for bit, all three branches: a window already S x S is a copy, a
 *  window exactly 2S x 2S takes the 2 x 2 mean, everything else the 11-bit fixed-point two-pass rule (tap positions in double, not
 *  contracted; csrc/slice.hip states it).  The product by float(1.0 / 255.0) is what `.float() / 255` gives on the device, so the view
 *  of the window (0, 0, w, h) has the bits of the plain predictor's input.
 *  TAMTR_EINVAL: a NULL operand, h, w, V or S < 1, a window that is empty or leaves the frame.  TAMTR_EUNSUP: V > 64 (the windows
 *  travel as a kernel argument), S > 65535 (grid y).
 *
 * tamtr_slice_merge: every view's rows mapped to its frame and merged by tamtr_tta_merge's rule, for a batch in one launch, one
 * workgroup per frame.
 *      y        (dtype) [N, nq, 4 + nc]  the eval outputs of all views of the batch: cx cy w h in 0..1 of the view, class scores
 *      view_off HOST i32 [B + 1]  frame b owns views view_off[b] .. view_off[b + 1] - 1; view_off[0] = 0, view_off[B] = N, every frame
 *                                 owns at least one view (checked here, passed by value)
 *      views    f32 [N, 4]        ox oy kx ky per view: cx' = cx kx + ox; cy' = cy ky + oy; w' = w kx; h' = h ky.  The caller computes
 *                                 them in double and rounds once: ox = x0 / w, kx = (x1 - x0) / w, likewise for y; (0, 0, 1, 1) is the identity
 *      match    0: IoU, torchvision's arithmetic; 1: IoS = inter / min(area_a, area_b); both suppress on `> iou` in fp32, NaN never does
 *      classes  i32 [n_classes] or NULL (no class filter)
 *      ym       f32 [B, max_out, 4 + nc]  the first max_out NMS survivors in order: cx' cy' w' h', the source row's scores; zero rows after
 *      src      i32 [B, max_out]  the candidate i = v_local nq + q a row came from, -1 after counts[b]
 *      counts   i32 [B]           rows written
 *      dropped  i32 [B]           survivors that did not fit into max_out rows
 *      overflow i32 [B]           candidates that passed the filter beyond the table of 4096 (the highest i), left out of the merge
 *  Bit-exact in fp32, every operation rounded on its own: class max, `score > conf`, the class filter, the passing candidates compacted
 *  in ascending i into a table of 4096, order by descending score (equal scores: ascending i), greedy class-aware NMS (shift
 *  cls * max_wh unless single_cls).  Nothing is written past a table; nothing is allocated, set or synchronised, so the call can be captured.
 *  TAMTR_EINVAL: a NULL operand, N, B, nq or max_out < 1, nd < 5, n_classes < 0, dtype not F32 / BF16, match not 0 / 1, a view_off
 *  that does not start at 0, end at N or gives a frame no view.  TAMTR_EUNSUP: B > 255, a frame with more than 64 views, nq > 512,
 *  max_out > 512. */
int tamtr_slice_views(const uint8_t* src, int h, int w, const int32_t* windows, int V, int S, float* out, void* stream);
int tamtr_slice_merge(const void* y, int dtype, int N, int B, int nq, int nd, const int32_t* view_off, const float* views, int match,
                      float conf, float iou, int single_cls, float max_wh, const int32_t* classes, int n_classes, int max_out, float* ym,
                      int32_t* src, int32_t* counts, int32_t* dropped, int32_t* overflow, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAMTR_HIP_H */
