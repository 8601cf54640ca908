/*
 * myolo_hip_internal.h -- stage-level entry points of libmyolo_hip.so used by the engine (mask-yolo_amd/myolo/engine.py) to
 * compose its fused pipelines: the Winograd transform / multiply stages, conv gradients that form a BatchNorm gradient lazily,
 * row-sparse helpers of the exact-sparsity backward, batched frozen-BatchNorm coefficients.  Same C-ABI conventions as
 * myolo_hip.h (caller-owned buffers, explicit stream, status codes), but the V / M / U / Q buffers exchanged between these
 * calls have LIBRARY-OWNED layouts ("opaque"): they are only meaningful to the matching stage of the same library build.
 * A maintainer replacing a Keras layer binds the operators of myolo_hip.h, not these.
 */
#ifndef MYOLO_HIP_INTERNAL_H
#define MYOLO_HIP_INTERNAL_H

#include "myolo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- frozen BatchNorm coefficients of many layers in one launch (inference trunk) ---- */
/* the same coefficients for many layers in one launch: table [nlayers][6] int64 (device) = element offsets of gamma, beta into params,
 * of the moving mean, moving variance into stats, of the layer's output into coeffs (scale[C] then shift[C]), and C */
int myolo_bn_frozen_coeffs_batched(const float* params, const float* stats, const int64_t* table, int nlayers, float* coeffs,
                                   void* stream);

/* frozen BatchNormalization (training=False, model.py:696,702,708) + ReLU/ReLU6 backward from the POST-activation tensor
 * a = act(gamma*xhat + beta): where the activation passes gradient xhat = (a - beta)/gamma, so the pre-BN tensor is not needed.
 * dx = scale * dy * [act passes], dgamma = sum dz*xhat, dbeta = sum dz.  ws as bn_act_bwd. */
int myolo_bn_act_bwd_frozen_post(const float* dy, const float* a_post, const float* gamma, const float* beta, const float* scale,
                                 float* dx, float* dgamma, float* dbeta, int64_t M, int C, int act,
                                 void* ws, size_t ws_bytes, void* stream);

/* ---- prepared-weights registry: the weight-only re-layouts that entry points run in front of their kernels (transposes, bf16x6 piece splits, Winograd
 * filter transforms) recorded once and re-run by the owner on a stream of its choice, off the training step's critical chain (csrc/myolo_common.h).
 * arena: a 256-byte aligned device buffer the slots are carved from (entries that do not fit stay on the in-place path).  activate(h) makes h the
 * registry the entry points consult (NULL: none); refresh re-runs entries [first, last) on `stream` for the current weight generation and returns
 * how many it launched; invalidate: the weights changed.  One launch thread per process. ---- */
int myolo_wprep_create(void* arena, size_t arena_bytes, void** handle);
int myolo_wprep_destroy(void* h);
int myolo_wprep_activate(void* h);
int myolo_wprep_count(void* h);
int myolo_wprep_invalidate(void* h);
int myolo_wprep_refresh(void* h, int first, int last, int max_idle, void* stream);
int myolo_wprep_stats(void* h, long long* hits, long long* misses, long long* bytes_used);
int myolo_wprep_overflows(void* h, long long* n);      /* resolve() calls whose new site found no room in the arena (made in place every step, never recorded) */

/* Exact-sparsity helpers for the mask head backward (build_mask_graph model.py:690-708: bn1 is the only
 * batch-statistics layer, so behind it only ROIs with a positive target carry non-zero gradient):
 * gather_groups: dst[i] = src[idx[i]] for groups of group_elems floats (one ROI's rows);
 * bn_act_bwd_rowsparse: training-mode BN+activation backward where the upstream gradient is given only
 *   for the n_groups row groups idx[] (compact dy [n_groups*group_rows, C]; inv[group] = slot or -1);
 *   results are identical to bn_act_bwd on the zero-padded dense gradient. */
int myolo_gather_groups(const float* src, const int32_t* idx, float* dst, int n, int64_t group_elems, void* stream);
/* the index those helpers take, built on the device from the per-image positive counts of myolo_mask_targets (an image's positives are its first
 * n_pos[b] ROIs, model.py:593): flags [B*R] (NULL: not written) = 1 for a positive ROI, inv [B*R] = its compact slot or -1, idx [slot] = flat ROI
 * (the first sum(n_pos) entries of a [B*R] buffer are written), total [1] (NULL: not written) = sum(n_pos).  No host round trip. */
int myolo_positive_index(const int32_t* n_pos, int B, int R, int32_t* flags, int32_t* idx, int32_t* inv, int32_t* total, void* stream);
/* myolo_deconv2x2s2_mask_fwd (include/myolo_hip.h) that ALSO writes relu(deconv + bias) -- exactly what myolo_deconv2x2s2_fwd(ACT_RELU) gives -- for the images (ROIs) the training step will
 * differentiate: keep_inv [N] = slot (0 <= slot < keep_cap) or -1 (myolo_positive_index), keep_d [keep_cap][2H][2W][Cout]; images whose slot is -1 or
 * >= keep_cap are not kept.  Needs Cout % 256 == 0 (the matrix-pipe kernels of csrc/wino_mm.hip). */
int myolo_deconv2x2s2_mask_fwd_keep(const float* x, const float* w, const float* bias, const float* w2, const float* b2, float* p_out,
                                    int N, int H, int W, int Cin, int Cout, int ncls, const int32_t* keep_inv, float* keep_d, int keep_cap,
                                    void* ws, size_t ws_bytes, void* stream);
/* the same gather of n groups of group_rows x C floats, fused with the per-channel affine map + activation that follows it in the compacted mask-head
 * backward: dst_pre (NULL: not written) = the gathered rows, dst_act = act(row * scale + shift) as myolo_bn_apply_act gives.  C / 4 must divide 256. */
int myolo_gather_groups_affine_act(const float* src, const int32_t* idx, const float* scale, const float* shift, int act, float* dst_pre,
                                   float* dst_act, int n, int64_t group_rows, int C, void* stream);
int myolo_bn_act_bwd_rowsparse(const float* dy_compact, const float* x, const int32_t* idx, const int32_t* inv,
                               const float* mean, const float* var, const float* scale, const float* shift,
                               float* dx, float* dgamma, float* dbeta,
                               int64_t M, int C, int n_groups, int group_rows, int act,
                               void* ws, size_t ws_bytes, void* stream);

/* ---- Winograd F(4,3)/F(2,3) tiling: buffer sizes and the forward's stages (csrc/wino_kernels.hip) ---- */
/* elements of the 36 transformed planes V (or M) of an [N,H,W,C] tensor (<= 36*N*ceil(H/4)*ceil(W/4)*C: with mixed tiling --
 * F(2,3) on a last tile row / column that holds <= 2 outputs, e.g. 14 = 4+4+4+2 -- reduced tiles have no row in the planes of
 * the points they do not use; at 14x14 that is 484 instead of 576 point-tiles per image) */
size_t myolo_wino_plane_elems(int N, int H, int W, int C);
/* floats to allocate for U of myolo_wino_weight_transform (1.5 x 36*Cin*Cout: room for the split-bf16 layout of option "wino_x6") */
size_t myolo_wino_u_elems(int Cin, int Cout);

/* the forward's four stages, callable on their own: U = 36 planes of Cin*Cout transformed filter taps (flip=1: of the rotated
 * filter with the channel roles exchanged, for the data gradient: call the multiply with (Cout, Cin) then).  U is OPAQUE between
 * myolo_wino_weight_transform and myolo_wino_multiply: the element order inside a plane is the one the multiply kernel chosen
 * for (Cin, Cout) wants ([K][N], or [N][K] for csrc/wino_mm.hip when K % 16 == 0 and N % 256 == 0).  V and M = 36 planes of myolo_wino_plane_elems(N,H,W,C) elements in total (a buffer of 36*T*C floats,
 * T = N*ceil(H/4)*ceil(W/4), always suffices); planes are ordered by point group, see csrc/wino_kernels.hip */
int myolo_wino_weight_transform(const float* w, float* U, int Cin, int Cout, int flip, void* stream);
int myolo_wino_input_transform(const float* x, float* V, int N, int H, int W, int C, void* stream);
int myolo_wino_multiply(const float* V, const float* U, float* M, int N, int H, int W, int Cin, int Cout, void* stream);
/* weight_transform (flip 0) + multiply; U_scratch is written only when the filters are not already prepared for this step (myolo_wprep_*) */
int myolo_wino_multiply_w(const float* V, const float* w, float* U_scratch, float* M, int N, int H, int W, int Cin, int Cout, void* stream);
int myolo_wino_output_transform(const float* M, const float* bias, const float* scale, const float* shift, float* y,
                                int N, int H, int W, int C, int act, void* stream);
/* ROIAlign (myolo_crop_and_resize_fwd: same boxes / box_ind / sampling) fused into the input transform of the conv that
 * consumes the crops: V [36][nb*ceil(crop_h/4)*ceil(crop_w/4)][C] directly from the feature map [B,FH,FW,C] */
int myolo_wino_input_transform_roialign(const float* feature, const float* boxes, const int32_t* box_ind, float* V, int B, int FH, int FW,
                                        int C, int nb, int crop_h, int crop_w, void* stream);
/* input transform with the producing layer's BatchNorm apply + activation folded into the load (scale/shift per channel) */
int myolo_wino_input_transform_affine(const float* x, const float* scale, const float* shift, int act, float* V, int N, int H, int W,
                                      int C, void* stream);
/* output transform (+bias) that also produces the training-mode BatchNorm statistics of what it writes: same outputs as
 * myolo_bn_stats (mean, var, folded scale/shift, moving averages; model.py:690).  C/4 must divide 256. */
size_t myolo_wino_output_transform_bn_ws_bytes(int C);
int myolo_wino_output_transform_bn_stats(const float* M, const float* bias, float* y, int N, int H, int W, int C, const float* gamma,
                                         const float* beta, float* mean, float* var, float* scale, float* shift, float* moving_mean,
                                         float* moving_var, void* ws, size_t ws_bytes, void* stream);
/* conv gradients whose incoming gradient sits behind a training-mode BatchNorm + activation with a row-sparse upstream
 * gradient (bn1 of the mask head, model.py:690 -- only the positive ROIs carry gradient, myolo_mask_loss_graph
 * model.py:739-746): bn_bwd_rowsparse_coeffs reduces dgamma / dbeta and leaves the per-channel terms ka, kb of
 * dx = scale*dz + ka + kb*x; the *_lazybn gradients form dx while loading the pre-BN tensor, so it is never written. */
int myolo_bn_bwd_rowsparse_coeffs(const float* dy_compact, const float* x, const int32_t* idx, const float* mean, const float* var,
                                  const float* scale, const float* shift, float* dgamma, float* dbeta, float* ka, float* kb, int64_t M,
                                  int C, int n_groups, int group_rows, int act, void* ws, size_t ws_bytes, void* stream);
int myolo_conv3x3_wino_bwd_data_lazybn(const float* y_pre, const float* dy_compact, const int32_t* inv, const float* scale,
                                       const float* shift, const float* ka, const float* kb, int act, const float* w, float* dx, int N,
                                       int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int myolo_conv3x3_wino_bwd_weight_lazybn(const float* v_saved, const float* y_pre, const float* dy_compact, const int32_t* inv,
                                         const float* scale, const float* shift, const float* ka, const float* kb, int act, float* dw,
                                         int N, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
/* layer boundary between two Winograd convs in one pass per image: M of conv_i -> (+bias, affine, act) -> V of conv_{i+1}
 * through LDS; the activation itself goes to y only for images with flags[img] != 0 (flags NULL: all; y NULL: none).
 * Needs C % 32 == 0 and ceil(H/4)*ceil(W/4) <= 32 (14x14: 16 tiles). */
int myolo_wino_output_input_transform(const float* M, const float* bias, const float* scale, const float* shift, float* y,
                                      const int32_t* flags, float* V_next, int N, int H, int W, int C, int act, void* stream);
/* ... writing the conv's PRE-BatchNorm output (A^T m A + bias) to ypre where flags[img] != 0 (NULL: everywhere) instead of the activation */
int myolo_wino_output_input_transform_keep_pre(const float* M, const float* bias, const float* scale, const float* shift, float* ypre,
                                               const int32_t* flags, float* V_next, int N, int H, int W, int C, int act, void* stream);

/* ---- trunk backward: BatchNorm-backward sums from the producer of the BatchNorm's output gradient (csrc/mem_kernels.hip) ---- */
/* The same data gradient when dx is the gradient reaching a TRAINING-mode BatchNorm + activation (the conv_pw_{b-1}_bn / conv1_bn in front of this
 * depthwise conv, model.py:51,68-77): xbn = that BatchNorm's pre-BN tensor [N,H,W,C], scale / shift / mean / var = its forward coefficients.  The
 * kernel also leaves the BatchNorm backward's sums (sum dz, sum dz * xhat) as `rows` rows of [2][C] double partials in `part`;
 * myolo_bn_act_bwd_from_partials finishes them (fixed order) and forms the BatchNorm's dx -- the pass over (dx, xbn) myolo_bn_act_bwd starts with
 * is gone.  rows = myolo_dwconv3x3_bwd_data_bnsums_rows(...); 0 = not available for these sizes (use the two plain calls). */
int myolo_dwconv3x3_bwd_data_bnsums_rows(int N, int H, int W, int C, int stride);
int myolo_dwconv3x3_bwd_data_bnsums(const float* dy, const float* w, float* dx, int N, int H, int W, int C, int stride, const float* xbn,
                                    const float* scale, const float* shift, const float* mean, const float* var, int act, double* part, int rows,
                                    void* stream);
/* myolo_bn_act_bwd(batch_stats = 1) from sums a producer already left as nblk rows of [2][C] double partials (myolo_dwconv3x3_bwd_data_bnsums):
 * finish in row order -> dgamma, dbeta; then dx.  ws: 2 * C doubles. */
int myolo_bn_act_bwd_from_partials(const float* dy, const float* x, const float* mean, const float* var, const float* scale, const float* shift,
                                   float* dx, float* dgamma, float* dbeta, int64_t M, int C, int act, const double* part, int nblk,
                                   void* ws, size_t ws_bytes, void* stream);

/* ---- F(6,3)/F(4,3) tiling of 14x14 maps: buffer sizes and stages (csrc/wino63_kernels.hip) ---- */
size_t myolo_wino63_plane_elems(int N, int C);
size_t myolo_wino63_u_elems(int Cin, int Cout);

int myolo_wino63_weight_transform(const float* w, float* U, int Cin, int Cout, void* stream);
int myolo_wino63_multiply(const float* V, const float* U, float* M, int N, int Cin, int Cout, void* stream);
/* weight_transform + multiply in one call (w = the layer's [3,3,Cin,Cout] kernel): U_scratch (myolo_wino63_u_elems floats) is written only when the
 * transformed filters are not already prepared for this step (prepared-weights registry, myolo_wprep_* above) */
int myolo_wino63_multiply_w(const float* V, const float* w, float* U_scratch, float* M, int N, int Cin, int Cout, void* stream);
/* x [N,14,14,C] -> a = act(x*scale + shift) (scale NULL: identity) -> V.
 * keep (NULL: nothing kept) receives a's rows of the selected images:
 *   keep_cap == 0: keep_sel = flags [N] (NULL: every image); keep is dense, [N,14,14,C];
 *   keep_cap  > 0: keep_sel = slots [N] (myolo_positive_index: compact slot of an image or -1), required; keep is compact -- the rows of image n sit at
 *                  block slots[n] when 0 <= slots[n] < keep_cap, so the sparse mask-head backward needs no gather */
int myolo_wino63_input_transform(const float* x, const float* scale, const float* shift, int act,
                                 float* keep, const int32_t* keep_sel, int keep_cap,
                                 float* V, int N, int C, void* stream);
/* layer boundary in one kernel: M -> pre = A^T m A + bias -> a = act(pre*scale + shift) -> Vn (NULL: no next conv, a plain output transform).
 * y (NULL: not written): a, every image.
 * keep (NULL: nothing kept): rows of the selected images (keep_sel / keep_cap as above), pre if keep_pre else a.  pre is the conv's PRE-BatchNorm output:
 * the exact-sparsity backward reads bn2-4's backward off it.  MYOLO_EINVAL for y && keep && !keep_pre (the kernel has a single activation output) and
 * for a call with nothing to write */
int myolo_wino63_boundary(const float* M, const float* bias, const float* scale, const float* shift, int act,
                          float* y, float* keep, int keep_pre, const int32_t* keep_sel, int keep_cap,
                          float* Vn, int N, int C, void* stream);
/* conv1 of the mask head on this tiling: ROIAlign fused into the input transform (myolo_wino_input_transform_roialign), the output
 * transform that also yields the training-mode BatchNorm statistics (myolo_wino_output_transform_bn_stats), and the weight gradient
 * from the kept V planes and the lazily formed output gradient (myolo_conv3x3_wino_bwd_weight_lazybn) */
int myolo_wino63_input_transform_roialign(const float* feature, const float* boxes, const int32_t* box_ind, float* V, int B, int FH, int FW,
                                          int C, int nb, void* stream);
size_t myolo_wino63_output_transform_bn_ws_bytes(int N, int C);
int myolo_wino63_output_transform_bn_stats(const float* M, const float* bias, float* y, int N, int C, const float* gamma, const float* beta,
                                           float* mean, float* var, float* scale, float* shift, float* moving_mean, float* moving_var,
                                           void* ws, size_t ws_bytes, void* stream);
size_t myolo_wino63_bwd_weight_ws_bytes(int N, int Cin, int Cout);
int myolo_wino63_bwd_weight_lazybn(const float* v_saved, const float* y_pre, const float* dy_compact, const int32_t* inv, const float* scale,
                                   const float* shift, const float* ka, const float* kb, int act, float* dw, int N, int Cin, int Cout,
                                   void* ws, size_t ws_bytes, void* stream);
/* conv1's backward with ONE pass over y_pre: the lazily formed gradient of the conv's output is transformed both ways in one kernel --
 * V (operand of the data gradient) and Q (operand of the weight gradient), myolo_wino63_plane_elems(N, C) floats each -- and the two
 * gradients are finished by the calls below (on different streams if the caller likes: they share nothing but read-only inputs).
 * Same results as myolo_wino63_bwd_data_lazybn + myolo_wino63_bwd_weight_lazybn, bit for bit. */
int myolo_wino63_lazybn_transforms(const float* y_pre, const float* dy_compact, const int32_t* inv, const float* scale, const float* shift,
                                   const float* ka, const float* kb, int act, float* V, float* Q, int N, int C, void* stream);
size_t myolo_wino63_bwd_data_from_v_ws_bytes(int N, int Cin, int Cout);
int myolo_wino63_bwd_data_from_v(const float* V, const float* w, float* dx, int N, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
size_t myolo_wino63_bwd_weight_from_q_ws_bytes(int N, int Cin, int Cout);
int myolo_wino63_bwd_weight_from_q(const float* v_saved, const float* Q, float* dw, int N, int Cin, int Cout, void* ws, size_t ws_bytes,
                                   void* stream);

/* The plane-wise weight-gradient product behind myolo_wino63_bwd_weight_from_q and the F(4,3) chain under "wino_x6", by itself: for up to 4 runs of
 * planes (run r: nq[r] planes of rows[r] rows each, packed one after another in run order in A [rows][Ka] and B [rows][N]), C[plane] (Ka x N) =
 * A[plane]^T B[plane] with six exact bf16 piece products per fp32 product.  rows / nq are HOST arrays; runs with 0 rows or 0 planes are skipped.
 * Ka, N multiples of 256.  MYOLO_EWORKSPACE when ws is smaller than the split plan's partial tiles. */
int myolo_gemm_tn_bf16x6_planes(const float* A, const float* B, float* C, int nruns, const int64_t* rows, const int32_t* nq, int Ka, int N,
                                void* ws, size_t ws_bytes, void* stream);
/* myolo_deconv2x2s2_bwd_weight on the same product whatever the number of pixels (the public entry takes it from 4096 input pixels under "wino_x6"):
 * the four taps of dy gathered into the A operand.  Cin and 4 Cout multiples of 256. */
int myolo_deconv2x2s2_bwd_weight_bf16x6(const float* x, const float* dy, float* dw, int N, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes,
                                        void* stream);

/* myolo_conv3x3_wino_bwd_data_lazybn on this tiling (same operands; needs myolo_wino63_ok(14, 14, Cout, Cin)) */
size_t myolo_wino63_bwd_data_ws_bytes(int N, int Cin, int Cout);
int myolo_wino63_bwd_data_lazybn(const float* y_pre, const float* dy_compact, const int32_t* inv, const float* scale, const float* shift,
                                 const float* ka, const float* kb, int act, const float* w, float* dx, int N, int Cin, int Cout, void* ws,
                                 size_t ws_bytes, void* stream);
/* ---- training-mode BatchNorm fusion of the trunk (model.py:42-79, 249-278 with every BatchNormalization on batch statistics):
 * "*_bnstats_fwd" = the conv AND the batch statistics of its output (mean, biased variance, folded scale / shift, Keras moving averages:
 * exactly what myolo_bn_stats produces) -- the statistics are reduced from partial sums the conv kernel leaves in its epilogue, so the
 * output is not re-read; "in_scale / in_shift / in_act" = the PRODUCING layer's BatchNorm apply + activation, performed on the load of
 * its pre-BN output, so the normalised activation is never written (NULL: the input is used as it is).  "phases": 3 = both launches
 * (the conv, then the statistics finish); 1 / 2 = only the first / second, for callers that bracket the conv kernel with events.  The "*_bwd_weight_affine_in"
 * gradients re-normalise the same pre-BN tensor on load.  Results equal the unfused sequences up to fp32 summation order. ---- */
/* inference: act(conv(x) * scale + shift) in one launch: the frozen conv1_bn + ReLU6 folded into the conv's store (scale / shift from
 * myolo_bn_frozen_coeffs[_batched]); bit-identical to myolo_conv3x3s2_c3_fwd + myolo_bn_apply_act (model.py:45-52, BatchNormalization in inference mode) */
int myolo_conv3x3s2_c3_affine_act_fwd(const float* x, const float* w, const float* scale, const float* shift, int act, float* y,
                                      int N, int H, int W, int Cout, void* stream);
size_t myolo_conv3x3s2_c3_bnstats_ws_bytes(int N, int H, int W, int Cout);
int myolo_conv3x3s2_c3_bnstats_fwd(const float* x, const float* w, float* y, const float* gamma, const float* beta, float* mean, float* var,
                                   float* scale, float* shift, float* moving_mean, float* moving_var, int N, int H, int W, int Cout, int phases,
                                   void* ws, size_t ws_bytes, void* stream);
size_t myolo_dwconv3x3_bnstats_ws_bytes(int N, int H, int W, int C, int stride);
int myolo_dwconv3x3_bnstats_fwd(const float* x, const float* in_scale, const float* in_shift, int in_act, const float* w, float* y,
                                const float* gamma, const float* beta, float* mean, float* var, float* scale, float* shift,
                                float* moving_mean, float* moving_var, int N, int H, int W, int C, int stride, int phases,
                                void* ws, size_t ws_bytes, void* stream);
int myolo_dwconv3x3_bwd_weight_affine_in(const float* x, const float* in_scale, const float* in_shift, int in_act, const float* dy, float* dw,
                                         int N, int H, int W, int C, int stride, void* ws, size_t ws_bytes, void* stream);
int    myolo_pwconv1x1_bnstats_ok(int Cin, int Cout);
size_t myolo_pwconv1x1_bnstats_ws_bytes(int64_t M, int Cin, int Cout);
int myolo_pwconv1x1_bnstats_fwd(const float* x, const float* in_scale, const float* in_shift, int in_act, const float* w, float* y,
                                const float* gamma, const float* beta, float* mean, float* var, float* scale, float* shift,
                                float* moving_mean, float* moving_var, int64_t M, int Cin, int Cout, int phases, void* ws, size_t ws_bytes, void* stream);
int myolo_pwconv1x1_bwd_weight_affine_in(const float* x, const float* in_scale, const float* in_shift, int in_act, const float* dy, float* dw,
                                         int64_t M, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);

/* ---- the mask loss and the mask conv 1x1's backward for any class count (myolo_mask_loss_graph model.py:718-754 reads one channel per ROI:
 * class_id of a positive ROI), myolo_mask_head_out_bwd's dense dz [M,C] being limited to C <= 8.
 * mask_bce_sel: myolo_mask_bce's inputs and loss_out (bit-identical loss) but only the gradient of the selected channel,
 *   dz_sel [NR*h*w] = dz[r, ids[r / (h*w)]] (0 for a ROI whose id is not in 1..C-1).  ws: as myolo_mask_bce.
 * mask_head_out_bwd_sel: x [M,Cin] (the ReLU'd deconv output), w [Cin,C], dz_sel [M], ids [M/hw] (class per ROI of hw rows):
 *   dx[r,c] = (x[r,c] > 0) ? dz_sel[r] * w[c, ids[r/hw]] : 0 (bit-identical to myolo_mask_head_out_bwd on the one-hot dz);
 *   dw[Cin,C], db[C] = sums over the rows of the ROIs of each class, in doubles, ROI order: every column is written, a class
 *   without a ROI gets zeros.  Needs Cin / 4 dividing 256.  ws: myolo_mask_head_out_bwd_sel_ws_bytes(M/hw, Cin). ---- */
int myolo_mask_bce_sel(const float* target_masks, const int32_t* target_class_ids, const float* pred, float loss_weight,
                       float* loss_out, float* dz_sel, int NR, int h, int w, int C, void* ws, size_t ws_bytes, void* stream);
size_t myolo_mask_head_out_bwd_sel_ws_bytes(int NR, int Cin);
int myolo_mask_head_out_bwd_sel(const float* x, const float* w, const float* dz_sel, const int32_t* ids, float* dx, float* dw, float* db,
                                int64_t M, int Cin, int C, int hw, void* ws, size_t ws_bytes, void* stream);

/* ---- HBM stream-copy microbenchmark (the measured copy bandwidth printed beside the nominal 8 TB/s): dst = src over
 * nbytes (multiple of 16), hand-written float4 kernel, 4 loads in flight per thread.  variant 0 default cache policy, 1 non-temporal
 * stores, 2 non-temporal loads + stores, 3 read only, 4 write only; blocks <= 0: 8 workgroups per CU. ---- */
int myolo_stream_copy(const void* src, void* dst, size_t nbytes, int variant, int blocks, void* stream);
/* Matrix-pipe ceiling probe: `blocks` workgroups of four waves (<= 0: 512 = two per CU), each wave `iters` rounds of eight independent
 * accumulator blocks from register operands.  kind 0: v_mfma_f32_32x32x16_bf16 (32768 flop each), kind 1: v_mfma_f32_32x32x2_f32 (4096 flop each),
 * kind 2 / 3: bf16 with the eight issues of a round on two alternating / one accumulator block (dependent-issue chains).
 * flop per launch = blocks * 4 * iters * 8 * flop-per-instruction.  `out` (blocks * 256 floats) is practically never written. */
int myolo_mfma_probe(int kind, int iters, int blocks, float* out, void* stream);

/* ---- ResNet-50 backbone (cfg.BACKBONE = "resnet50": keras_applications ResNet50 v1) : csrc/resnet_kernels.hip.  Declared here rather than in
 * the operator API (myolo_hip.h, held to 70 entries): the engine composes the ResNet trunk from these and the existing operators ----
 * conv1: ZeroPadding2D(3) + Conv2D 7x7 stride 2 'valid', 3 -> Cout, + bias; x [N,H,W,3], y [N,Ho,Wo,Cout], Ho = (H-1)/2+1.  An EXPLICIT im2col
 *   ([M][160] fp32 in ws: K = 147 taps, column 147 = 1 meeting the bias as row 147 of the padded weights) followed by the pointwise MFMA GEMMs;
 *   ws >= myolo_conv7x7s2_c3_ws_bytes (at 16 x 512^2: 671 MB of im2col matrix, written and read back by the forward and again by the weight
 *   gradient).  _bnstats_fwd: training form, the GEMM's epilogue leaves the column sums of y (bias included) and the finish writes mean / var /
 *   scale / shift and updates the moving statistics (as myolo_bn_stats).  _affine_act_fwd: inference form, act((conv + bias)*scale + shift) in the
 *   GEMM's store.  bwd_weight writes dw [7,7,3,Cout] and (if non-NULL) db [Cout] (per-workgroup partials, fixed-order reduction: deterministic). */
size_t myolo_conv7x7s2_c3_ws_bytes(int N, int H, int W, int Cout);
int myolo_conv7x7s2_c3_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cout,
                           void* ws, size_t ws_bytes, void* stream);
int myolo_conv7x7s2_c3_bnstats_fwd(const float* x, const float* w, const float* bias, float* y, const float* gamma, const float* beta, float* mean,
                                   float* var, float* scale, float* shift, float* moving_mean, float* moving_var, int N, int H, int W, int Cout,
                                   void* ws, size_t ws_bytes, void* stream);
int myolo_conv7x7s2_c3_affine_act_fwd(const float* x, const float* w, const float* bias, const float* scale, const float* shift, int act, float* y,
                                      int N, int H, int W, int Cout, void* ws, size_t ws_bytes, void* stream);
int myolo_conv7x7s2_c3_bwd_weight(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cout,
                                  void* ws, size_t ws_bytes, void* stream);
/* ZeroPadding2D(1) + MaxPool2D 3x3 stride 2 'valid' of act(x*scale + shift) (scale = shift = NULL: of x; the training step folds bn_conv1's
 * apply + ReLU into this load).  y [N,Ho,Wo,C], arg [N,Ho,Wo,C] uint8 = row-major window index 0..8 of the first maximum (a padding cell, value 0,
 * can win).  bwd: dx [N,H,W,C] = sum over the <= 4 windows that chose the pixel, in window order; a gradient routed to padding is dropped. */
int myolo_maxpool3x3s2_fwd(const float* x, const float* scale, const float* shift, int act, float* y, uint8_t* arg,
                           int N, int H, int W, int C, void* stream);
int myolo_maxpool3x3s2_bwd(const float* dy, const uint8_t* arg, float* dx, int N, int H, int W, int C, void* stream);
/* strided 1x1 convs: xs [N,(H-1)/2+1,(W-1)/2+1,C] = x at the even rows / columns; scatter: dx [N,H,W,C] = a + b there (b may be NULL), 0 elsewhere */
int myolo_gather_s2(const float* x, float* xs, int N, int H, int W, int C, void* stream);
int myolo_scatter_s2(const float* a, const float* b, float* dx, int N, int H, int W, int C, void* stream);
/* residual join: out = ReLU(y*scale + shift + r), r = sc*sc_scale + sc_shift (projection block) or sc (identity: sc_scale = sc_shift = NULL);
 * bwd: g = dout * [out > 0] (the gradient of both BatchNorm inputs and, in an identity block, of the block input through the shortcut) */
int myolo_residual_fwd(const float* y, const float* scale, const float* shift, const float* sc, const float* sc_scale, const float* sc_shift,
                       float* out, int64_t M, int C, void* stream);
int myolo_residual_bwd(const float* dout, const float* out, float* g, int64_t n, void* stream);

/* ---- evaluation (myolo/evaluate.py): pixel overlaps between the PASTED masks of selected detections and ground-truth planes, counted on the
 * device -- the paste of myolo_unmold_masks (same device function, same pixels) without writing or downloading a full-size mask.  Declared here
 * rather than in the operator API (myolo_hip.h, held to 70 entries).
 * masks [B,R,mh,mw,C] and det [B,R,6] as the inference graph returns them; sel [B,K] int32 (device) = the rows of det chosen per image, < 0 = empty
 * slot, K <= 16; sel_host = the same [B,K] values in host memory, read before anything is launched (a value >= R is refused: the selection is made
 * on the host from the downloaded detections, so the caller has them); gt_masks [B,H,W,T] uint8 0 / 1, T <= 32.
 * inter [B,K,T] = pixels set in both pasted mask k and plane t; area_pred [B,K], area_gt [B,T] = pixels set in each; win [B,K,4] = the clamped
 * pixel window [x1,y1,x2,y2) of the paste; all int32, zeros for an empty slot.  Integer atomics only: bit-identical from run to run.
 * ws: B * K int32. */
int myolo_mask_overlap_counts(const float* masks, const float* det, const int32_t* sel, const int32_t* sel_host, const uint8_t* gt_masks,
                              int32_t* inter, int32_t* area_pred, int32_t* area_gt, int32_t* win, int B, int R, int K, int T, int mh, int mw,
                              int C, int H, int W, void* ws, size_t ws_bytes, void* stream);

/* ---- detection masks as run-length codes (myolo/rle.py, MaskYOLO.detect(mask_format="rle"); format and kernels: DESIGN.md section 15): the PASTED
 * masks of selected detections -- the paste of myolo_unmold_masks, the same device function, pixel for pixel -- as the boundaries of COCO's
 * run-length form, without writing or downloading a full-size mask.  Declared here rather than in the operator API (myolo_hip.h, held to 70 entries).
 * masks, det, sel, sel_host as myolo_mask_overlap_counts takes them (K <= 16, sel < 0 = empty slot, a value >= R refused); frames [B,2] int32 =
 * (h, w) of image b's output frame, on the device and (frames_host) in host memory: every image has its own.  sel_host and frames_host are read
 * before anything is launched.
 * With the pixels of a mask in column-major order, p = x * h + y, a boundary is every p in [0, h * w) whose pixel differs from pixel p - 1 (pixel -1
 * counts as 0): bounds[run_off[s] .. run_off[s + 1]) are the boundaries of slot s = b * K + k, ascending (positions, not lengths: COCO's counts are
 * diff([0, boundaries..., h * w])); an empty slot has none.  run_off [B*K+1] is always written in full; nothing is written at or beyond
 * bounds + cap, so a caller that finds run_off[B*K] > cap grows its buffer and calls again.  Integer work only: bit-identical from run to run.
 * MYOLO_EINVAL (message "rle_masks: ...", nothing written) for a null pointer, K > 16, h or w < 1, h * w >= 2^31, sel >= R, and a workspace under
 * myolo_rle_masks_ws_bytes(B, K, max_w), max_w = the widest frame of the call (a workspace planned for narrower frames is refused). */
size_t myolo_rle_masks_ws_bytes(int B, int K, int max_w);
int myolo_rle_masks(const float* masks /*[B,R,mh,mw,C]*/, const float* det /*[B,R,6]*/,
                    const int32_t* sel /*[B,K] device, <0 = empty*/, const int32_t* sel_host,
                    const int32_t* frames /*[B,2] device: h, w of image b's output frame*/, const int32_t* frames_host,
                    int32_t* run_off /*[B*K+1]*/, uint32_t* bounds /*[cap]*/, int64_t cap,
                    int B, int R, int K, int mh, int mw, int C, void* ws, size_t ws_bytes, void* stream);

/* ---- detection masks as polygons (myolo/contour.py, MaskYOLO.detect(mask_format="polygon"); contract and kernels: DESIGN.md section 21): the closed
 * loops that bound the PASTED masks of selected detections -- the paste of myolo_unmold_masks, the same device function, pixel for pixel -- as
 * vertex lists in lattice corner coordinates (pixel (y, x) is the square [x, x+1] x [y, y+1]), traced on the device without writing or downloading
 * a full-size mask.  Declared here rather than in the operator API (myolo_hip.h, held to 70 entries).
 * masks, det, sel, sel_host, frames, frames_host as myolo_rle_masks takes them.  verts[vert_off[s] .. vert_off[s + 1]) are the vertices (X, Y) of
 * slot s = b * K + k in contour.trace's order: loops ascending by their smallest edge key (Y, X, dir), each from the start corner of that edge in
 * traversal order with the inside on the right; loop_id is the ordinal of each vertex's loop within its slot (from 0, never decreasing inside a
 * slot).  An empty slot has no vertex.  vert_off [B*K+1] is always written in full; nothing is written at or beyond cap vertices, and when
 * vert_off[B*K] > cap NO vertex is written: the caller grows verts, loop_id and the workspace and calls again.  Integer work only behind the
 * paste: bit-identical from run to run.
 * MYOLO_EINVAL (message "contour_masks: ...", nothing launched) for a null pointer, K > 16, h or w < 1, h * w >= 2^31, 2^30 corners x slots in the
 * batch, sel >= R, cap outside [0, 2^31), and a workspace that is not 8-byte aligned or lies under myolo_contour_masks_ws_bytes(B, K, max_h,
 * max_w, cap), max_h / max_w = the tallest / widest frame of the call.  The workspace holds 4 * B * K bytes per row of max_h and 44 bytes per
 * vertex of cap; it does not grow with the frame's area. */
size_t myolo_contour_masks_ws_bytes(int B, int K, int max_h, int max_w, int64_t cap);
int myolo_contour_masks(const float* masks /*[B,R,mh,mw,C]*/, const float* det /*[B,R,6]*/,
                        const int32_t* sel /*[B,K] device, <0 = empty*/, const int32_t* sel_host,
                        const int32_t* frames /*[B,2] device: h, w of image b's output frame*/, const int32_t* frames_host,
                        int32_t* vert_off /*[B*K+1]*/, int32_t* verts /*[cap][2]: X, Y*/, int32_t* loop_id /*[cap]*/, int64_t cap,
                        int B, int R, int K, int mh, int mw, int C, void* ws, size_t ws_bytes, void* stream);

/* ---- measurements of the detected instances (myolo/measure.py, MaskYOLO.detect(measure=True); the record and the kernel: DESIGN.md section 25):
 * for the PASTED mask of every selected detection -- the paste of myolo_unmold_masks, the same device function, pixel for pixel -- a record of
 * MYOLO_MEASURE_WORDS exact integer sums, taken on the device without writing or downloading a full-size mask.  Declared here rather than in the
 * operator API (myolo_hip.h, held to 70 entries).
 * masks, det, sel, sel_host, frames, frames_host as myolo_rle_masks takes them, but K is 1 .. 128, taken whole: a slot is ranked against ALL
 * earlier slots of its image.  A slot value may repeat a row.  With m(x, y) the mask of slot s = b * K + k over image b's h x w frame (x the
 * column, y the row; 0 outside the frame), out[s] is
 *   0 area, 1 visible_area = the set pixels that no earlier live slot of the image holds, 2 sx, 3 sy, 4 sxx, 5 syy, 6 sxy = the sums of x, y,
 *   x*x, y*y, x*y over the set pixels, 7 perimeter = the unit edges between a set pixel and a 4-neighbour that is 0 or outside the frame,
 *   8 quads = the positions with m(x,y) & m(x+1,y) & m(x,y+1) & m(x+1,y+1), 9 .. 12 x1, y1, x2, y2 = the tight box of the set pixels, far corner
 *   exclusive, zeros when area is 0;
 * an empty slot (sel < 0) is 13 zeros.  Every word of out is written (the caller zeroes nothing), nothing behind out or behind ws_bytes, and the
 * result does not depend on what the workspace held.  h, w <= 32768 keep every word inside int64.  Integer work only behind the paste, 64-bit
 * integer atomics across workgroups: bit-identical from run to run.
 * MYOLO_EINVAL (message "measure_masks: ...", nothing launched, out untouched) for a null pointer, B < 1, K outside 1 .. 128, h or w outside
 * 1 .. 32768, sel >= R, and a workspace under myolo_measure_masks_ws_bytes(B, K).  sel_host and frames_host are read before anything is
 * launched. */
#define MYOLO_MEASURE_WORDS 13
size_t myolo_measure_masks_ws_bytes(int B, int K);
int myolo_measure_masks(const float* masks /*[B,R,mh,mw,C]*/, const float* det /*[B,R,6]*/,
                        const int32_t* sel /*[B,K] device, <0 = empty*/, const int32_t* sel_host,
                        const int32_t* frames /*[B,2] device: h, w*/, const int32_t* frames_host,
                        int64_t* out /*[B,K,13]*/, int B, int R, int K, int mh, int mw, int C,
                        void* ws, size_t ws_bytes, void* stream);

/* ---- overlay of the selected detections (myolo/render.py, MaskYOLO.detect(render=True); the picture and the kernel: DESIGN.md section 16): the
 * three layers of render.render_instances -- every PASTED mask blended into the image, every mask's one-pixel outline, the dashed ring of every
 * paste window, each over the slots in order -- drawn from the uploaded image bytes in one launch.  A mask pixel is the paste of
 * myolo_unmold_masks (the same device function), so out is render_instances of the dense paste byte for byte; no dense mask is written or
 * downloaded.  Declared here rather than in the operator API (myolo_hip.h, held to 70 entries).
 * images: the pack_images layout -- desc [B,3] int64 = (byte offset from images, h, w) of image b, on the device and (desc_host) in host memory;
 * nbytes = the bytes of the batch behind images (< 2^31), which every image must lie within.  A batch at one size is the descriptor of B equal
 * images over a [B,H,W,3] tensor.  out: uint8 in the same layout at the same offsets (nbytes too; the bytes between images are not touched); two
 * descriptors must not name overlapping bytes.  masks, det, sel, sel_host as myolo_mask_overlap_counts takes them (image b pastes into its own
 * h x w frame; K <= 16, sel < 0 = empty slot, a value >= R refused); colors [B,K,3] double in [0, 1] (device).
 * flags: bit 0 the blend, bit 1 the outline, bit 2 the box.  The blend is canvas * (1 - alpha) + (alpha * colour) * 255 in double, each product and
 * the sum rounded on its own, truncated to the canvas; box_alpha takes alpha's place in the ring.
 * MYOLO_EINVAL (message "render_instances: ...", nothing launched) for a null pointer, K outside 1 .. 16, sel >= R, h or w < 1, an image beyond
 * nbytes, nbytes >= 2^31, alpha or box_alpha outside [0, 1], and a workspace under B * K int32.  desc_host and sel_host are read before anything
 * is launched. */
int myolo_render_instances(const uint8_t* images, uint8_t* out, size_t nbytes,
                           const int64_t* desc /*[B,3] device: offset, h, w*/, const int64_t* desc_host,
                           const float* masks /*[B,R,mh,mw,C]*/, const float* det /*[B,R,6]*/,
                           const int32_t* sel /*[B,K] device, <0 = empty*/, const int32_t* sel_host,
                           const double* colors /*[B,K,3] device*/, double alpha, double box_alpha, int flags,
                           int B, int R, int K, int mh, int mw, int C, void* ws, size_t ws_bytes, void* stream);

/* ---- on-device training augmentation (myolo/augment.py, csrc/augment_kernels.hip; arithmetic contract: DESIGN.md "On-device augmentation").
 * Declared here rather than in the operator API (myolo_hip.h, held to 70 entries).  Per image b one row of params: the INVERSE affine map
 * (output pixel -> source position, pixel-centre convention baked into m02 / m12), then gain and bias of the byte values.  The image is sampled
 * bilinearly (a tap outside the frame reads cval), the instance masks by nearest neighbour; a live source instance (class id != 0) whose warped
 * mask is empty is dropped and the survivors are compacted in order; gt_boxes = extract_bboxes of the warped masks; y_true / true_boxes =
 * BatchGenerator._encode of those boxes (both NULL: not written).  Every output element is written.  T <= 32.
 * ws: myolo_augment_batch_ws_bytes(B, T). */
size_t myolo_augment_batch_ws_bytes(int B, int T);
int myolo_augment_batch(const uint8_t* src_images,   /* [B,H,W,3] */
                        const uint8_t* src_masks,    /* [B,H,W,T] 0/1 */
                        const int32_t* src_class_ids,/* [B,T], 0 = empty slot */
                        const double*  params,       /* [B,8]: m00 m01 m02 m10 m11 m12 gain bias */
                        double cval, const double* anchors /* [2A] */,
                        float* images, uint8_t* gt_masks, int32_t* gt_boxes, int32_t* gt_class_ids,
                        float* y_true /* [B,G,G,A,5+C], or NULL with true_boxes */, float* true_boxes /* [B,T,4] */,
                        int B, int H, int W, int T, int G, int A, int C,
                        void* ws, size_t ws_bytes, void* stream);

/* ---- mosaic (myolo/augment.py: Mosaic; arithmetic contract: DESIGN.md "Mosaic").  myolo_augment_batch with four tiles per output image: pixel
 * (x, y) of image b lies in tile q = (x >= cx) + 2 * (y >= cy), (cx, cy) = centre[b], and is sampled from image quad_src[b][q] of the same batch
 * through the row quad_rows[b][q] by the formulas above.  The instance candidates of an image are the 4T pairs (q, t) in q-major order, live iff
 * src_class_ids[quad_src[b][q]][t] != 0; a candidate covers a pixel of tile q whose source mask tap is set; a candidate with no pixel is dropped,
 * the first T survivors fill slots 0..T-1 in order, the others are discarded (their pixels are in no output mask) and counted in dropped[b].
 * Boxes, ids and targets as above.  With quad_src[b] = {b,b,b,b}, quad_rows[b][q] = params[b] and centre (W, H) every output equals
 * myolo_augment_batch's byte for byte.  The tables are device memory and are NOT read on the host: the caller (DeviceAugmenter) refuses sources
 * outside [0, B) and centres outside [0, W] x [0, H] before it uploads them; the kernels only keep a bad source index from becoming an address.
 * T <= 32.  ws: myolo_mosaic_batch_ws_bytes(B, T). */
size_t myolo_mosaic_batch_ws_bytes(int B, int T);
int myolo_mosaic_batch(const uint8_t* src_images,   /* [B,H,W,3] */
                       const uint8_t* src_masks,    /* [B,H,W,T] 0/1 */
                       const int32_t* src_class_ids,/* [B,T], 0 = empty slot */
                       const int32_t* quad_src,     /* [B,4] batch positions */
                       const double*  quad_rows,    /* [B,4,8]: a params row per tile */
                       const int32_t* centre,       /* [B,2]: cx, cy */
                       double cval, const double* anchors /* [2A] */,
                       float* images, uint8_t* gt_masks, int32_t* gt_boxes, int32_t* gt_class_ids,
                       float* y_true /* [B,G,G,A,5+C], or NULL with true_boxes */, float* true_boxes /* [B,T,4] */,
                       int32_t* dropped /* [B] */,
                       int B, int H, int W, int T, int G, int A, int C,
                       void* ws, size_t ws_bytes, void* stream);

/* ---- copy-paste (myolo/augment.py: CopyPaste; contract: DESIGN.md "Copy-paste").  A second stage behind myolo_augment_batch / myolo_mosaic_batch,
 * on their outputs: image b receives instances of image d = donor[b] of the same batch.  live(i,t) = src_class_ids[i][t] != 0; S = the slots t,
 * ascending, with bit t of select[b] set and live(d,t) (empty when d is outside [0, B): the index never becomes an address); A = the first
 * F = T - #{t: live(b,t)} of S; dropped[b] = |S| - |A|, and a rejected instance is not pasted at all.  U(x,y) = some t in A has src_masks[d,y,x,t]
 * != 0.  Pixel (x,y) of images[b] is the three floats of src_images[d] under U and of src_images[b] elsewhere, copied bit for bit.  The 2T
 * candidates are the own slots (live(b,t); pixels src_masks[b,y,x,t] != 0 outside U), then the donor's (t in A; pixels src_masks[d,y,x,t] != 0); one
 * with no pixel is dropped (not counted), the survivors fill slots 0.. in order.  Masks are 0/1, unused slots zero; boxes, ids and targets as above.
 * With select all zero, and inputs as the first stage writes them, every output equals the input byte for byte.  No output may lie over an input: a
 * donor is read in its state before the paste.  The tables are device memory and are NOT read on the host (augment.check_paste_tables).
 * MYOLO_EINVAL (message "copy_paste_batch: ...", nothing launched or written) for a null pointer (y_true and true_boxes: together or not at all),
 * bad sizes, T > 32, an output over an input and a workspace under myolo_copy_paste_batch_ws_bytes(B, T). */
size_t myolo_copy_paste_batch_ws_bytes(int B, int T);
int myolo_copy_paste_batch(const float*   src_images,   /* [B,H,W,3] */
                           const uint8_t* src_masks,    /* [B,H,W,T] 0/1 */
                           const int32_t* src_class_ids,/* [B,T], 0 = empty slot */
                           const int32_t* donor,        /* [B] batch positions */
                           const int32_t* select,       /* [B] bit t: donor slot t is selected */
                           const double* anchors /* [2A] */,
                           float* images, uint8_t* gt_masks, int32_t* gt_boxes, int32_t* gt_class_ids,
                           float* y_true /* [B,G,G,A,5+C], or NULL with true_boxes */, float* true_boxes /* [B,T,4] */,
                           int32_t* dropped /* [B] */,
                           int B, int H, int W, int T, int G, int A, int C,
                           void* ws, size_t ws_bytes, void* stream);

/* ---- photometric augmentation (myolo/augment.py: Photometric; contract: DESIGN.md section 26, csrc/photometric_kernels.hip).  The last stage of
 * the device augmenter, on the float image of the stage before it.  Row p = rows[b] holds 32 doubles: [0:12] a 3x4 colour transform A, row major;
 * [12] the noise deviation; [13] the noise key, an integer in [0, 2^32); [14] the blur radius r, an integer in 0..15; [15] 0; [16:32] the blur
 * weights w_0..w_15.  With r' = min(r, max_radius), s the input as doubles and refl reflect-101 (refl(i,1) = 0):  h = w0*s(x,y), then for k =
 * 1..r' ascending h = h + w_k*(s(refl(x-k,W),y) + s(refl(x+k,W),y));  v the same over y on h (h stays binary64);  u_c = ((A[c][0]*v_0 +
 * A[c][1]*v_1) + A[c][2]*v_2) + A[c][3];  u_c = u_c + p[12]*n with n = ((double)S - 131070.0) * (1.7320508075688772 / 65536.0), S the sum of the
 * four 16-bit fields of splitmix64((key << 32) | ((y*W + x)*3 + c));  images = (float)(u_c > 0 ? (u_c < 1 ? u_c : 1) : 0).  Every operation is one
 * binary64 operation in this order, none fused.  On the identity row ([I|0], 0, 0, 0, 0, w_0 = 1) the output has the input's bits.
 * rows is device memory and is NOT read on the host (augment.check_photo_rows).  max_radius, 0..15, is the caller's host-known bound: a row never
 * widens a loop beyond it; with max_radius = 0 no blur pass is launched and no workspace is needed (ws may be NULL).
 * MYOLO_EINVAL (message "photometric_batch: ...", nothing launched or written) for a null pointer, B, H, W <= 0 (or H*W*3 >= 2^31 - 256, B > 65535),
 * max_radius outside 0..15, an output over the input or the rows, and a workspace under myolo_photometric_batch_ws_bytes(B, H, W, max_radius). */
size_t myolo_photometric_batch_ws_bytes(int B, int H, int W, int max_radius);
int myolo_photometric_batch(const float* src_images /* [B,H,W,3] */, const double* rows /* [B,32], device */,
                            float* images /* [B,H,W,3] */, int max_radius, int B, int H, int W,
                            void* ws, size_t ws_bytes, void* stream);

/* ---- inference input of any size (MaskYOLO.detect / detect_many, csrc/resize_kernels.hip; arithmetic contract: DESIGN.md section 14).  Declared here
 * rather than in the operator API (myolo_hip.h, held to 70 entries).  B uint8 [h,w,3] images of mixed sizes, packed back to back in src at ANY byte
 * offset, resized to the network frame: per image and channel myolo_utils.resize(image, (H, W), preserve_range=True).astype(uint8) in binary64 --
 * pixel centres aligned, taps floor / ceil, a tap outside the source reads 0, clipped to the minimum / maximum byte of the whole source image --
 * bit for bit; out_unit = (float)((double)u8 / 255.), as myolo_u8_to_unit_f32 forms it.  Two launches: per-image min / max, then the samples.
 * MYOLO_EINVAL (message "resize_images: ...") for a null pointer, B, H, W <= 0, h or w < 1, an image that does not lie inside src_bytes (read from
 * desc_host before anything is launched) and a workspace under myolo_resize_images_ws_bytes(B). */
size_t myolo_resize_images_ws_bytes(int B);
int myolo_resize_images_u8(const uint8_t* src, size_t src_bytes,
                           const int64_t* desc,      /* device [B,3]: byte offset into src, h, w of image b ([h,w,3] uint8, dense) */
                           const int64_t* desc_host, /* the same values in host memory */
                           uint8_t* out_u8,          /* [B,H,W,3] or NULL */
                           float* out_unit,          /* [B,H,W,3] or NULL; at least one of the two */
                           int B, int H, int W, void* ws, size_t ws_bytes, void* stream);

/* ---- segment rasteriser (myolo/coco.py and myolo/via.py datasets, csrc/segment_kernels.hip; contract: DESIGN.md sections 13 and 18).  Declared
 * here rather than in the operator API (myolo_hip.h, held to 70 entries).  Fills the annotations of a batch into the instance masks
 * myolo_augment_batch reads: the slot b*T+t holds any number of polygon parts (a VIA outline is one part) and / or one run-length code, and
 * masks[b,i,j,t] = 1 when source pixel (r, c) = (src_row[b,i], src_col[b,j]) is ON in any of the slot's parts -- skimage.draw.polygon (0.18.3)
 * lists it for that part; every part with its own start vertex, parities and vertex flag: a union, not even-odd across parts -- or when the number
 * of the slot's boundaries <= c * src_h[b] + r is odd.  A slot with neither parts nor boundaries is empty (an all-zero code has no boundary, an
 * all-one code the single boundary 0).  The two tables are made on the host by the rule of resize_mask (the identity for an image already at
 * network size); they only name pixels inside the source frame, which is all the frame clipping there is.  No limit on parts, vertices, runs or T;
 * the offsets are trusted (the callers build them: myolo_utils.pack_segments).  boxes, when given, receives the tight box of
 * every slot's set pixels in the output frame (integer atomicMin / atomicMax: the same from run to run).
 * MYOLO_EINVAL (message "segment_masks: ...", nothing launched) for a null pointer other than verts, bounds and boxes, and for B, H, W, T <= 0. */
int myolo_segment_masks(const double* verts,        /* [n_verts,2] (row, col), source-image pixels; may be NULL when there is no part */
                        const int32_t* part_off,    /* [n_parts+1] offsets into verts */
                        const int32_t* slot_part,   /* [B*T+1] offsets into part_off: the parts of slot k */
                        const int32_t* bounds,      /* [n_bounds] running sums of a code's counts without the final total, ascending, duplicates allowed */
                        const int32_t* slot_bound,  /* [B*T+1] offsets into bounds */
                        const int32_t* src_h,       /* [B] source image height (the stride of p = col * h + row) */
                        const int32_t* src_row,     /* [B,H] source row that output row i samples */
                        const int32_t* src_col,     /* [B,W] */
                        uint8_t* masks,             /* [B,H,W,T] 0/1, EVERY element written */
                        int32_t* boxes,             /* [B,T,4] x1,y1,x2,y2 (far corner exclusive), 0,0,0,0 for a slot without a set pixel; or NULL */
                        int B, int H, int W, int T, void* stream);

/* ---- anchor fitting (myolo/anchors.py, csrc/anchors_kernels.hip; contract: DESIGN.md section 19).  Declared here rather than in the operator API
 * (myolo_hip.h, held to 70 entries).  k-means over box sizes with 1 - IoU as the distance, `runs` independent runs in ONE call: run r has its own
 * k = run_k[r] (1 .. 32) and its own initial centroids (w, h) in centroids[r, 0 .. k), which the call replaces by the fitted ones (rows >= k are not
 * touched).  All in binary64 without contraction: inter = min(w, cw) * min(h, ch), iou = inter / ((w * h + cw * ch) - inter), d = 1.0 - iou, a point
 * goes to the lowest index of the smallest d.  After an assignment pass that changed nothing the run is converged; otherwise a non-empty cluster's
 * centroid becomes (double)sum / (double)count (64-bit integer sums: exact, the same bits from run to run) and an EMPTY cluster keeps its centroid.
 * iterations = assignment passes made (<= max_iter); converged = 0 for a run that max_iter stopped: its centroids are those of the last update.
 * counts and assign (NULL: not written) are the last pass's; mean_iou = the mean over the points of the largest IoU against the final centroids,
 * summed from per-workgroup partials in index order (no floating-point atomics).
 * wh, centroids, counts, iterations, converged, mean_iou, assign, ws are DEVICE pointers, wh holding values >= 1; run_k is read on the host before
 * anything is launched.  The host drives the passes (one pair of launches each, a finished run's workgroups return at once, its flags are read every
 * few passes), and the call SYNCHRONISES the stream before it returns: the outputs are final then.
 * MYOLO_EINVAL (message "anchor_kmeans: ...", nothing launched) for a null pointer other than assign, n < 1, runs < 1, a k outside 1 .. 32,
 * max_iter < 1, and a workspace under myolo_anchor_kmeans_ws_bytes(n, runs). */
size_t myolo_anchor_kmeans_ws_bytes(int64_t n, int runs);
int    myolo_anchor_kmeans(const int32_t* wh /*[n,2] device*/, int64_t n, const int32_t* run_k /*host [runs]*/,
                           double* centroids /*[runs,32,2] in/out*/, int runs, int max_iter, int64_t* counts /*[runs,32]*/,
                           int32_t* iterations /*[runs]*/, int32_t* converged /*[runs]*/, double* mean_iou /*[runs]*/,
                           int32_t* assign /*[runs,n] or NULL*/, void* ws, size_t ws_bytes, void* stream);

/* ---- detect()'s selection on the device (myolo/detect.py: select with its 10 replaced by K; csrc/select_kernels.hip; contract: DESIGN.md section
 * 23).  Declared here rather than in the operator API (myolo_hip.h, held to 70 entries).  det [B,R,6] float32 as the inference graph returns it
 * (x1, y1, x2, y2 normalised, score, class id); one workgroup per image, every decision the host's, bit for bit:
 *   1. a row is live when (x2 - x1) * (y2 - y1) > 0 in binary32 (two subtractions and a product, not contracted; both extents negative is live);
 *   2. the live rows in descending score, ties by the HIGHER row first (np.argsort(scores, kind="stable")[::-1]); the first K of them;
 *   3. of those the rows with (double)score >= cs_threshold, in order: the list L;
 *   4. entry j of L is dropped when ANY earlier entry i of L, dropped or not, has the same class, (int32)det[5] by truncation, and
 *      IoU >= nms_threshold: myolo_utils.bbox_iou_2 in binary64 -- corners (double)x * shape0 and (double)y * shape1 (image_shape[0] and [1], in
 *      that order), _interval_overlap's branches as written, inter / ((w1 * h1 + w2 * h2) - inter); a zero denominator (the host raises) does not
 *      suppress;
 *   5. the survivors, in order.
 * sel [B,K] int32 = their rows of det[b], -1 in the empty slots; picked [B,K,6] = det[b, sel[b,k]] bit for bit, zeros in the empty slots;
 * count [B] = survivors per image.  An image b >= n_live only gets its -1s, zeros and count 0.  Scores are finite by construction (a sigmoid
 * product): a non-finite score is outside the contract.  Nothing is read back: no synchronisation.
 * MYOLO_EINVAL (message "select_detections: ...", nothing launched) for a null pointer, B < 1, K outside 1 .. 128, R outside 1 .. 4096 and
 * n_live outside 0 .. B. */
int myolo_select_detections(const float* det /*[B,R,6]*/, int B, int R, int n_live, int K, double cs_threshold, double nms_threshold,
                            int shape0, int shape1, int32_t* sel /*[B,K]*/, float* picked /*[B,K,6]*/, int32_t* count /*[B]*/, void* stream);

/* ---- the training recipe's optimiser pass (myolo/optim.py, Net.recipe_step; csrc/optim_kernels.hip; contract: DESIGN.md section 24): global-norm
 * gradient clipping, AdamW's decoupled weight decay, a freeze mask and an EMA shadow of the weights in ONE read of p, g, m, v, behind a
 * deterministic gradient-norm reduction; nothing comes back to the host.  They belong beside myolo_adam_step and are declared here only because
 * the operator API (myolo_hip.h) is held to 70 entries.  All buffers are flat float32 of n elements, n % 4 == 0, 16-byte aligned.
 *   flags [n/4] uint8, one byte per group of four consecutive elements: bit 0 = trainable, bit 1 = decayed.
 *   stats: a 24-byte device record { double sumsq; float norm; float scale; int32 skipped; int32 steps; } (zero it once).
 * myolo_grad_sumsq: sumsq = sum over the trainable groups of (double)x * (double)x, x = g[i] * gs in binary32; per-thread double sums combined in
 *   a fixed order (workgroup tree, then the partials in one workgroup: a grid that depends on n only, no float atomics), so the bits repeat from
 *   run to run and agree between ranks that hold the same gradient.  norm = (float)sqrt(sumsq).  scale = 1.0f when clip == 0 (off) or
 *   sumsq <= (double)clip * clip, else (float)((double)clip / sqrt(sumsq)); a NaN or infinite sumsq gives scale = 0 and skipped += 1 (the step is
 *   skipped); steps += 1 always.  partials: MYOLO_OPTIM_PARTIALS doubles of scratch.
 * myolo_adamw_ema_step: reads scale and the skip decision (sumsq not finite) from stats.  Skipped: nothing is written.  A group without bit 0:
 *   p, m, v, ema are not written.  Otherwise per element, every line one binary32 operation:
 *     gi = (g*gs)*scale;  mi = b1*m + (1-b1)*gi;  vi = b2*v + ((1-b2)*gi)*gi;  pn = p - (lr_t*mi)/(sqrtf(vi)+eps);
 *     decayed: pn = pn - lr_wd*p (the old p);  ema (nullable): ema = ema_d*ema + ema_omd*pn.
 * myolo_swap_f32: exchanges the contents of a and b in one pass.
 * MYOLO_EINVAL (nothing launched) for a null pointer (ema excepted), n <= 0, n % 4 != 0 and a negative or non-finite clip. */
#define MYOLO_OPTIM_PARTIALS 1024
int myolo_grad_sumsq(const float* g, const uint8_t* flags, int64_t n, float gs, float clip, void* stats, double* partials, void* stream);
int myolo_adamw_ema_step(float* p, const float* g, float* m, float* v, float* ema_or_null, const uint8_t* flags, int64_t n, const void* stats,
                         float lr_t, float b1, float b2, float eps, float gs, float lr_wd, float ema_d, float ema_omd, void* stream);
int myolo_swap_f32(float* a, float* b, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MYOLO_HIP_INTERNAL_H */
