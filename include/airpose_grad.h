/* airpose_grad.h -- C ABI of libairpose_grad.so (gfx950 / MI355X): the gradient entry points.
 *
 * The training-side companion of libairpose_hip.so.  It holds the forward / backward of the IEF regressor head
 * (copenet.forward_reg, copenet/src/copenet/models/model_copenet.py:178-204) and of the ResNet-50 trunk
 * (copenet.forward_feat_ext, model_copenet.py:161-176, train- or eval-mode BatchNorm) on live weights, and the adjoints of the
 * geometry helpers of the reference's training loss (copenet_twoview.py:205-317).  A library of its own, so that the
 * inference library's ABI, exports and binary stay as they are.
 *
 * Conventions
 *   - stateless: no handle.  Every data pointer is a DEVICE pointer owned by the caller (PyTorch's caching allocator);
 *     weights are read straight from the caller's fp32 row-major [out][in] storage on every call (no packing);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises;
 *   - return value: 0 = ok, negative = APG_E* argument error, positive = hipError_t; apg_last_error() returns a
 *     thread-local description;
 *   - no floating-point atomics: every reduction runs in a fixed order, so results are bit-reproducible run to run;
 *   - all tensors are dense row-major float32 unless stated.
 */
#ifndef AIRPOSE_GRAD_H
#define AIRPOSE_GRAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APG_OK 0
#define APG_EINVAL (-1) /* bad argument */
#define APG_ENOMEM (-4) /* workspace smaller than the query asked for */

/* ABI number of this header: bumped whenever an exported signature changes or an entry point is added or removed.
 * A binding built against another number must refuse to load the library (airpose_amd/_native_grad.py does). */
#define APG_ABI_VERSION 2
const char* apg_version(void);
int apg_abi_version(void);
const char* apg_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Dropout.  keep(seed, layer, row, col) <=> u >= p, u = 24-bit uniform of a counter-based hash of (seed, layer, row, col);
 * kept values are scaled by 1 / (1 - p).  layer 1 = drop1 (after fc1), 2 = drop2 (after fc2); row = view * B + sample.
 * p <= 0: every entry kept (the eval-mode identity).  Writes out[row][col] = keep ? 1 : 0 (uint8, rows x cols): exactly
 * the mask the head kernels apply. */
int apg_dropout_mask(uint64_t seed, int layer, int rows, int cols, float p, uint8_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * IEF regressor head, both views, R = 2B rows (view 0, then view 1).  fc1 input row (2332 columns):
 *   xc = [xf (2048) | bb (3) | pos (3) | orient (6) | art (126) | shape (10) | partner art (126) | partner shape (10)]
 * h1d = drop1(xc W1^T + b1), h2d = drop2(h1d W2^T + b2), delta = h2d [Wpose; Wshape]^T + [bpose; bshape],
 * pose = [pos | orient | art] + delta[:, :135], betas = shape + delta[:, 135:].
 *
 * apg_head_fwd
 *   state / state_ld: HOST arrays of 10 entries -- bb, pos, orient, art, shape of view 0, then of view 1: a device pointer
 *     and its row stride in floats (columns contiguous; stride 0 broadcasts one row to the B samples).
 *   xc (R x 2332), h1d (R x 1024), h2d (R x 1024): written; what apg_head_bwd reads (xc holds the snapshot of the state
 *     columns taken here, so the caller may change its inputs in place afterwards).
 *   pose_out / betas_out: HOST arrays of 2 device pointers (view 0, view 1), (B x 135) and (B x 10).
 *   p1, p2: dropout probabilities of drop1 / drop2 (0 when the module is not in training mode).
 * Matrix products on v_mfma_f32_16x16x4_f32 (exact fp32).  A sample's outputs depend only on its own row. */
int apg_head_fwd(int B, const float* xf0, const float* xf1, const void* const* state, const int* state_ld,
                 const float* W1, const float* b1, const float* W2, const float* b2, const float* Wpose, const float* bpose,
                 const float* Wshape, const float* bshape, uint64_t seed, float p1, float p2,
                 float* xc, float* h1d, float* h2d, void* const* pose_out, void* const* betas_out, void* stream);

/* Workspace of apg_head_bwd in bytes; need_gxf = 1 when the gradient of xf0 / xf1 is asked for. */
int64_t apg_head_bwd_workspace_bytes(int B, int need_gxf);

/* apg_head_bwd
 *   xc, h1d, h2d: what apg_head_fwd wrote; seed, p1, p2: the values it was given (the masks are regenerated).
 *   g_out: HOST array of 4 device pointers -- g_pose0 (B x 135), g_betas0 (B x 10), g_pose1, g_betas1; NULL = zero.
 *   g_param: HOST array of 8 device pointers -- gW1, gb1, gW2, gb2, gWpose, gbpose, gWshape, gbshape (each written, not
 *     accumulated; NULL = not needed).  Every entry is reduced over the R rows in a fixed order.
 *   g_in: HOST array of 12 device pointers -- g_xf, g_bb, g_pos, g_orient, g_art, g_shape of view 0, then of view 1,
 *     contiguous (B x width), written; NULL = not needed.  Each collects its own view's fc1 columns, the partner's
 *     art / shape columns (the fusion) and the identity of the residual, in that order.
 *   workspace: at least apg_head_bwd_workspace_bytes(B, g_xf0 || g_xf1) bytes. */
int apg_head_bwd(int B, const float* xc, const float* h1d, const float* h2d, const float* W1, const float* W2,
                 const float* Wpose, const float* Wshape, uint64_t seed, float p1, float p2, const void* const* g_out,
                 void* const* g_param, void* const* g_in, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Generic view-local head (head_local_grad.hip): ONE weight set over R rows, the layout given by the caller.  It serves
 * copenet.regressor_step (and copenet_sep), model_hmr, model_muhmr (both views as 2B rows) and model_copenet_singleview.
 *   xc = [xf (2048) | segment 0 | ... | segment nseg-1]        K1 = 2048 + S columns, S = the sum of the segment widths (K1 may be odd)
 *   h1d = drop1(xc W1^T + b1), h2d = drop2(h1d W2^T + b2)       W1 (1024 x K1), W2 (1024 x 1024)
 *   out_d = xc[:, 2048 + res_d : 2048 + res_d + n_d] + h2d W_d^T + b_d          for each decoder d, W_d (n_d x 1024)
 * Dropout rows are the row indices [0, R): apg_dropout_mask(seed, layer, R, 1024, p) is the mask.
 * Every product reduces over K in index order inside one workgroup and nothing uses atomics: results are bit-reproducible, and a
 * row's outputs and input gradients depend only on that row.
 *
 * apg_head_local_fwd
 *   seg / seg_ld / seg_w: HOST arrays of nseg (1 .. APG_HEAD_LOCAL_MAX_SEG) entries in fc1 column order -- device pointer, row
 *     stride in floats (columns contiguous; 0 broadcasts one row to the R rows; otherwise >= width) and width (1 .. 1024).
 *   dec_W / dec_b / dec_n / dec_res: HOST arrays of ndec (1 .. APG_HEAD_LOCAL_MAX_DEC) entries -- weight, bias, n_d (1 .. 1024) and
 *     the residual's first column counted from the first segment column; [res_d, res_d + n_d) must lie inside [0, S).
 *   xc (R x K1), h1d (R x 1024), h2d (R x 1024), wdec (N * 1025 floats, N = sum n_d: the packed (N x 1024)
 *     [W_0; W_1; ..] followed by the N packed biases): written; what apg_head_local_bwd reads.  xc and wdec are snapshots, so the
 *     caller may change its inputs in place afterwards.
 *   out: HOST array of ndec device pointers, (R x n_d) each.  All decoders run as ONE product of N columns.
 * Bad layouts (R < 1, too many segments or decoders, a residual range outside the segments, a NULL pointer) are APG_EINVAL. */
#define APG_HEAD_LOCAL_MAX_SEG 8
#define APG_HEAD_LOCAL_MAX_DEC 3
int apg_head_local_fwd(int R, const float* xf, int nseg, const void* const* seg, const int* seg_ld, const int* seg_w,
                       const float* W1, const float* b1, const float* W2, const float* b2, int ndec, const void* const* dec_W,
                       const void* const* dec_b, const int* dec_n, const int* dec_res, uint64_t seed, float p1, float p2,
                       float* xc, float* h1d, float* h2d, float* wdec, void* const* out, void* stream);

/* Workspace of apg_head_local_bwd in bytes for K1 fc1 columns and N decoder columns; need_gxf = 1 when g_xf is asked for.
 * Negative for a bad size. */
int64_t apg_head_local_bwd_workspace_bytes(int R, int K1, int N, int need_gxf);

/* apg_head_local_bwd
 *   seg_w, dec_n, dec_res: as in the forward call; seg_bcast[k] != 0: segment k was given with row stride 0, and its gradient is
 *     (1 x width): the sum over the R rows in row order (two fixed-order passes).
 *   xc, h1d, h2d, wdec: what apg_head_local_fwd wrote; seed, p1, p2: the values it was given (the masks are regenerated).
 *   g_out: HOST array of ndec device pointers, (R x n_d); NULL = zero.
 *   g_param: HOST array of 4 + 2 ndec device pointers -- gW1, gb1, gW2, gb2, then gW_d, gb_d per decoder (each written, not
 *     accumulated; NULL = not needed), reduced over the R rows in a fixed order.
 *   g_xf: (R x 2048), written; NULL = not needed (the feature columns of g_xc are then not computed).
 *   g_seg: HOST array of nseg device pointers, contiguous (R x width), or (1 x width) for a broadcast segment; written; NULL = not
 *     needed.  Each is the segment's fc1 columns of g_xc plus the output gradient of every decoder whose residual range holds the
 *     column, in decoder order.
 *   workspace: at least apg_head_local_bwd_workspace_bytes(R, K1, N, g_xf != NULL) bytes, else APG_ENOMEM. */
int apg_head_local_bwd(int R, int nseg, const int* seg_w, const int* seg_bcast, int ndec, const int* dec_n, const int* dec_res,
                       const float* xc, const float* h1d, const float* h2d, const float* wdec, const float* W1, const float* W2,
                       uint64_t seed, float p1, float p2, const void* const* g_out, void* const* g_param, float* g_xf,
                       void* const* g_seg, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Geometry adjoints (one workgroup per body for the per-body reductions, fixed order).
 *
 * rot6d_to_rotmat (copenet/src/copenet/utils/geometry.py:47-61, ap_rot6d_to_rotmat): x6 (n x 6), g_rotmat (n x 3 x 3)
 *   -> g_x6 (n x 6); the clamp_min(1e-12) of F.normalize included (below it the norm is a constant). */
int apg_rot6d_to_rotmat_bwd(const float* x6, int n, const float* g_rotmat, float* g_x6, void* stream);

/* perspective_projection (geometry.py:63-91, ap_perspective_projection): pts (B x P x 3), rotation (B x 3 x 3) or NULL
 * (identity), translation (B x 3) or NULL (zero), g_out (B x P x 2) -> g_pts (B x P x 3), g_rotation (B x 3 x 3),
 * g_translation (B x 3), g_center (B x 2); each output NULL = not needed. */
int apg_perspective_projection_bwd(const float* pts, int B, int P, const float* rotation, const float* translation, float fx,
                                   float fy, const float* g_out, float* g_pts, float* g_rotation, float* g_translation,
                                   float* g_center, void* stream);

/* transform_points (ap_transform_points, X' = R X + t): rt (B x 3 x 4), pts (B x P x 3), g_out (B x P x 3)
 *   -> g_rt (B x 3 x 4), g_pts (B x P x 3); each output NULL = not needed. */
int apg_transform_points_bwd(const float* rt, const float* pts, int B, int P, const float* g_out, float* g_rt, float* g_pts,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * ResNet-50 trunk primitives (trunk_grad.hip), one layer per call.  Activations are NHWC fp32 (n, H, W, C); conv weights are the
 * live OIHW fp32 parameters (K = C_out, C, R, S).  Products on v_mfma_f32_16x16x4_f32 (exact fp32), reductions in a fixed order.
 *
 * apg_conv_fwd: y (n, Ho, Wo, K) = conv(x, w), Ho = (H + 2 pad - R) / stride + 1 (likewise Wo).  The kernel must fit the
 * padded input, H + 2 pad >= R and W + 2 pad >= S, at every stride; otherwise every conv entry point returns APG_EINVAL and the
 * workspace query a negative size. */
int apg_conv_fwd(const float* x, int n, int H, int W, int C, const float* w, int K, int R, int S, int stride, int pad, float* y,
                 void* stream);

/* Workspace of apg_conv_bwd in bytes (the split-K partials of the weight gradient); negative for a bad geometry. */
int64_t apg_conv_bwd_workspace_bytes(int n, int H, int W, int C, int K, int R, int S, int stride, int pad);

/* apg_conv_bwd: gy (n, Ho, Wo, K), 16-byte aligned, K a multiple of 16 -> gx (n, H, W, C) and / or gw (K, C, R, S, written in OIHW);
 * each output NULL = not needed (at least one).  gx needs w, gw needs x and the workspace. */
int apg_conv_bwd(const float* x, int n, int H, int W, int C, const float* w, int K, int R, int S, int stride, int pad, const float* gy,
                 float* gx, float* gw, void* workspace, int64_t workspace_bytes, void* stream);

/* Workspace of apg_bn_fwd (train) / apg_bn_bwd over M = n H W rows of C channels, in bytes. */
int64_t apg_bn_workspace_bytes(int M, int C);

/* apg_bn_fwd: y = (x - mean) * invstd * gamma + beta (+ res) (ReLU when relu != 0) over x (M, C); y may alias x or res.
 *   train != 0: mean and the biased variance of the batch (per-tile centred partials combined by Chan's formula); when
 *     running_mean / running_var are given they are updated as nn.BatchNorm2d does: r = (1 - momentum) r + momentum * stat, with
 *     the unbiased variance (num_batches_tracked is the caller's).  Needs the workspace.
 *   train == 0: mean / var are running_mean / running_var (required, read only); no workspace.
 *   save_mean, save_invstd (C): written, what apg_bn_bwd reads (invstd = 1 / sqrt(var + eps)). */
int apg_bn_fwd(const float* x, int M, int C, const float* gamma, const float* beta, float* running_mean, float* running_var, int train,
               float momentum, float eps, const float* res, int relu, float* y, float* save_mean, float* save_invstd, void* workspace,
               int64_t workspace_bytes, void* stream);

/* apg_bn_bwd: gy (M, C) is the gradient of apg_bn_fwd's y; y (its output) gives the ReLU mask (NULL: no ReLU); x is its input.
 *   g = gy * (y > 0); gx = gamma invstd (g - mean(g) - xhat mean(g xhat)) (train) or gamma invstd g (eval); g_res = g (the residual's
 *   gradient; NULL = not needed); g_gamma = sum g xhat, g_beta = sum g (NULL = not needed).  gx may alias gy.  Needs the workspace. */
int apg_bn_bwd(const float* gy, const float* y, const float* x, int M, int C, const float* gamma, const float* save_mean,
               const float* save_invstd, int train, float* gx, float* g_res, float* g_gamma, float* g_beta, void* workspace,
               int64_t workspace_bytes, void* stream);

/* Max-pool 3 x 3 / s2 / p1 (padding = -inf): x (n, H, W, C) -> y (n, (H-1)/2+1, (W-1)/2+1, C).  Backward: each window's gradient goes to
 * its first maximum in row-major window order (torch's choice among ties); gx is written, not accumulated. */
int apg_maxpool_fwd(const float* x, int n, int H, int W, int C, float* y, void* stream);
int apg_maxpool_bwd(const float* x, int n, int H, int W, int C, const float* gy, float* gx, void* stream);

/* Avg-pool 7 x 7 of a (n, 7, 7, C) map -> (n, C), and its backward gx (n, 7, 7, C) = gy / 49. */
int apg_avgpool_fwd(const float* x, int n, int C, float* y, void* stream);
int apg_avgpool_bwd(const float* gy, int n, int C, float* gx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The trunk walker: the whole fixed [3, 4, 6, 3] graph, (n, 3, 224, 224) NCHW crops -> (n, 2048) features, in one call.
 *   params: HOST table of 53 x 5 device pointers, for each conv + BN pair in state_dict order (conv1 / bn1, then per bottleneck
 *     conv1 / bn1, conv2 / bn2, conv3 / bn3, downsample.0 / downsample.1): conv weight (OIHW), gamma, beta, running_mean, running_var.
 *   g_params: HOST table of 53 x 3 device pointers in the same order: gW (OIHW), g_gamma, g_beta; written, not accumulated; NULL =
 *     not needed.
 *
 * Workspace in bytes; save = 1: what apg_trunk_bwd reads (every conv output and BN output, per-channel mean and invstd, and the
 * backward's own buffers): 7.0 GB at n = 64 (about 110 MB per image); save = 0: forward only (five rotating activation buffers). */
int64_t apg_trunk_workspace_bytes(int n, int save);

/* apg_trunk_fwd: train != 0: BatchNorm on batch statistics, running_mean / running_var updated in place through the table (the
 * caller adds 1 to num_batches_tracked); train == 0: BatchNorm on the running statistics.  xf (n, 2048) written.  save = 1 keeps
 * what apg_trunk_bwd needs in the workspace.  1 <= n <= 2048. */
int apg_trunk_fwd(int n, const float* x, const void* const* params, int train, float momentum, float eps, float* xf, int save,
                  void* workspace, int64_t workspace_bytes, void* stream);

/* apg_trunk_bwd: after apg_trunk_fwd(save = 1) on the same workspace, n, train and parameters: g_xf (n, 2048) -> g_params and, when
 * g_x is not NULL, the gradient of the crops g_x (n, 3, 224, 224) NCHW. */
int apg_trunk_bwd(int n, const void* const* params, int train, const float* g_xf, void* const* g_params, float* g_x, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mixed-precision (bf16) training mode of the trunk (trunk_grad_bf16.hip).  Additive under ABI 2: a binding tells a library that
 * has these entry points from one that has not by looking up apg_trunk_precisions.
 *
 * Storage: activations and activation gradients are bf16 NHWC (passed as void*), every one 16-byte aligned with a channel count
 * that is a multiple of 8; parameters, parameter gradients, BatchNorm statistics, xf and the crop gradient are fp32.  Products are
 * bf16 x bf16 accumulated in fp32 (v_mfma_f32_16x16x32_bf16); each stored bf16 value is ONE round-to-nearest-even of an fp32 result.
 * Reductions run in a fixed order: results are bit-reproducible run to run.  A misaligned bf16 pointer or a channel count that is
 * not a multiple of 8 is APG_EINVAL, as are the geometry refusals of the fp32 entry points; a workspace smaller than its query
 * asks for is APG_ENOMEM, as in the fp32 entry points.  fp32 outputs (gw, an fp32 gx, statistics, xf) are written one float at a
 * time and need only their natural 4-byte alignment. */
#define APG_PREC_FP32 0
#define APG_PREC_BF16 1

/* Bit mask of the precisions the trunk walker takes: bit APG_PREC_FP32 | bit APG_PREC_BF16. */
int apg_trunk_precisions(void);

/* fp32 OIHW weights w (K, C, R, S) -> bf16 (RNE) in the two layouts the kernels read, input channels padded with zeros to Cp
 * (Cp >= C, a multiple of 8; K a multiple of 8): wf [K][R][S][Cp] (forward) and wd [Cp][R][S][K] (data gradient); either may be
 * NULL. */
int apg_pack_weights_bf16(const float* w, int K, int C, int Cp, int R, int S, void* wf, void* wd, void* stream);

/* y (n, Ho, Wo, K) bf16 = RNE(conv(x, w)): x (n, H, W, C) bf16, wf from apg_pack_weights_bf16 with Cp = C. */
int apg_conv_fwd_bf16(const void* x, int n, int H, int W, int C, const void* wf, int K, int R, int S, int stride, int pad, void* y,
                      void* stream);

/* Workspace of apg_conv_bwd_bf16 in bytes (the fp32 split-K partials, C padded channels wide); negative for a bad geometry. */
int64_t apg_conv_bwd_bf16_workspace_bytes(int n, int H, int W, int C, int K, int R, int S, int stride, int pad);

/* gy (n, Ho, Wo, K) bf16 -> gx (n, H, W, C) and / or gw; each output NULL = not needed (at least one).
 *   gx = RNE(dgrad(gy, wd) + add): wd from apg_pack_weights_bf16; add (same shape as gx, NULL = none; bf16, may alias gx, or with
 *     add_fp32 != 0 fp32, must not alias gx) is added in fp32 before the one rounding; gx_fp32 != 0: gx is written as fp32 instead
 *     (no add).  The walker keeps a downsample branch's data gradient in fp32 and hands it to conv1's data gradient as the fp32
 *     addend, so a block input's gradient is rounded once.
 *   gw (K, gw_channels, R, S) fp32 OIHW = the first gw_channels <= C input channels of wgrad(x, gy): fixed split-K chunks of fp32
 *     partials combined in chunk order; needs x and the workspace. */
int apg_conv_bwd_bf16(const void* x, int n, int H, int W, int C, const void* wd, int K, int R, int S, int stride, int pad, const void* gy,
                      const void* add, int add_fp32, void* gx, int gx_fp32, float* gw, int gw_channels, void* workspace, int64_t workspace_bytes,
                      void* stream);

/* BatchNorm on bf16 x / y / res / gy / gx / g_res; everything per channel is fp32.  Statistics are taken in fp32 from the stored
 * bf16 x with the tiles, partials and trees of apg_bn_fwd; arguments as apg_bn_fwd / apg_bn_bwd.  g_res is exact (gy or 0). */
int64_t apg_bn_bf16_workspace_bytes(int M, int C);
int apg_bn_fwd_bf16(const void* x, int M, int C, const float* gamma, const float* beta, float* running_mean, float* running_var, int train,
                    float momentum, float eps, const void* res, int relu, void* y, float* save_mean, float* save_invstd, void* workspace,
                    int64_t workspace_bytes, void* stream);
int apg_bn_bwd_bf16(const void* gy, const void* y, const void* x, int M, int C, const float* gamma, const float* save_mean,
                    const float* save_invstd, int train, void* gx, void* g_res, float* g_gamma, float* g_beta, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* The pools on bf16 maps.  Max-pool is a selection (exact); its backward sums a pixel's windows in fp32 and rounds once.
 * Avg-pool: bf16 (n, 7, 7, C) -> fp32 (n, C) summed in fp32 in row-major order; backward fp32 gy (n, C) -> bf16 gx = RNE(gy / 49). */
int apg_maxpool_fwd_bf16(const void* x, int n, int H, int W, int C, void* y, void* stream);
int apg_maxpool_bwd_bf16(const void* x, int n, int H, int W, int C, const void* gy, void* gx, void* stream);
int apg_avgpool_fwd_bf16(const void* x, int n, int C, float* y, void* stream);
int apg_avgpool_bwd_bf16(const float* gy, int n, int C, void* gx, void* stream);

/* The trunk walker with a precision argument.  APG_PREC_FP32 is apg_trunk_workspace_bytes / apg_trunk_fwd / apg_trunk_bwd, same
 * bits.  APG_PREC_BF16: x, params, g_params, xf, g_xf, g_x as there (all fp32); the crops are cast to bf16 (8 channels per pixel,
 * the last 5 zero), every conv weight is packed to bf16 into the workspace on every apg_trunk_fwd_p call (nothing is cached across
 * calls; the data gradient's packing only with save = 1) and apg_trunk_bwd_p reads that copy.  The workspace must be 256-byte aligned; save = 1: 3.7 GB at n = 64 (about 56 MB per
 * image and 94 MB of packed weights).  Any other precision: a negative size / APG_EINVAL. */
int64_t apg_trunk_workspace_bytes_p(int n, int save, int precision);
int apg_trunk_fwd_p(int precision, int n, const float* x, const void* const* params, int train, float momentum, float eps, float* xf,
                    int save, void* workspace, int64_t workspace_bytes, void* stream);
int apg_trunk_bwd_p(int precision, int n, const void* const* params, int train, const float* g_xf, void* const* g_params, float* g_x,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The training loss (loss_grad.hip): get_loss of the four reference trainers (copenet_twoview.py:83-161, copenet_singleview.py:
 * 76-117, hmr.py:75-116, muhmr.py:76-131) and the gradient of the total with respect to every prediction, in one pass.  Additive
 * under ABI 2: a binding tells a library that has it by looking up apg_loss_fwd_bwd.
 *
 * With m(x) the mean of x over all its elements, and per view v (summed over the views):
 *   trans          m((trans_v - gt_trans_v)^2)                                  (B x 3); absent when trans is NULL
 *   keypoints      m((j2d_v[:, :22] - gt_j2d_v[:, :22])^2)                      (B x 22 x 2)
 *   keypoints_3d   m(L3 * sum_v (joints_v[:, :22] - gt_joints[:, :22])^2 [+ (joints_0 - joints_1)^2])     ONE mean over B x 22 x 3;
 *                  L3 = limbs3d on joints {4, 5, 18, 19}, limbs3d^2 on {7, 8, 20, 21}, 1 elsewhere
 *   shape          m((verts_v - gt_verts)^2) [+ m((verts_0 - verts_1)^2)]       (B x V x 3)
 *   rootrot        m((rotmat_v[:, 0] - gt_root_v)^2)                            (B x 3 x 3)
 *   pose           m(LT * sum_v (rotmat_v[:, 1:] - gt_pose)^2 [+ (rotmat_0[:, 1:] - rotmat_1[:, 1:])^2])  ONE mean over B x 21 x 9;
 *                  LT = limbstheta on rotations {3, 4, 17, 18} of the 21, limbstheta^2 on {6, 7, 19, 20}
 *   betas          m(betas_v^2) [+ m((betas_0 - betas_1)^2)]                    (B x 10)
 *   cam            m(exp(-10 cam_v[:, 0])^2)                                    (B); absent when cam is NULL
 *   loss           scale * (w_trans trans + w_kp2d keypoints + w_kp3d keypoints_3d + w_shape shape + w_rootrot rootrot
 *                           + w_pose pose + w_beta betas + w_cam cam)
 * The bracketed cross-view shares exist with two views and their APG_LOSS_CROSS_* bit: the two-view trainer sets all four, muhmr
 * APG_LOSS_CROSS_POSE alone, the single-view trainer and hmr (nviews = 1) none.  The reference's scale is 60 and its w_cam is 1.
 *
 *   weights: HOST array of 11 floats, indexed by APG_LOSS_W_*.
 *   pred: HOST array of APG_LOSS_PER_VIEW * nviews device pointers; per view trans (B x 3), rotmat (B x 22 x 3 x 3), betas (B x 10),
 *     joints (B x J x 3), verts (B x V x 3), j2d (B x J x 2), cam (B x 3).  J >= 22; rows 22 .. J - 1 are never read.  trans and cam may
 *     be NULL (for both views or for neither); the others are required.  The two views may be the same pointers.
 *   gt: HOST array of 3 + 3 * nviews device pointers: gt_pose (B x 21 x 3 x 3), gt_joints (B x Jg x 3), gt_verts (B x V x 3), then per
 *     view gt_root (B x 3 x 3), gt_j2d (B x Jg x 2), gt_trans (B x 3; required when trans is given).  Jg >= 22.
 *   terms: 9 device floats, written in the order loss, trans, keypoints, keypoints_3d, shape, rootrot, pose, betas, cam; an absent term
 *     is written as 0.
 *   grads: NULL (no gradient: a forward-only call), or a HOST array of APG_LOSS_PER_VIEW * nviews device pointers in pred's order and
 *     shapes, each NULL = not needed.  Each given gradient is written in full, not accumulated: d loss / d input, rows >= 22 of
 *     g_joints / g_j2d and columns 1, 2 of g_cam as zeros.  A gradient of an absent trans / cam is APG_EINVAL.  No output may overlap
 *     an input or another output.
 *   workspace: at least apg_loss_workspace_bytes(B, V) bytes (negative for B < 1 or V < 1), else APG_ENOMEM; the per-workgroup
 *     partial sums.  It carries nothing from call to call and needs no initialisation.
 * Pointers need only their natural 4-byte alignment; when every vertex pointer is 16-byte aligned the vertex stream moves in 16-byte
 * accesses.  Determinism: no atomics; every sum is per-thread in index order, a fixed tree per workgroup, and the workgroups'
 * partials in index order.  The partition depends on (B, V, J) alone -- not on the pointers, their alignment or which gradients are
 * asked for -- so terms and gradients are bit-identical from run to run and from one such choice to another.
 * Two launches.  B < 1, V < 1, J < 22, Jg < 22, nviews outside {1, 2}, cross bits with nviews = 1 and a NULL required pointer are
 * APG_EINVAL before any launch. */
#define APG_LOSS_CROSS_JOINTS 1
#define APG_LOSS_CROSS_VERTS 2
#define APG_LOSS_CROSS_POSE 4
#define APG_LOSS_CROSS_BETAS 8
#define APG_LOSS_CROSS_ALL 15
#define APG_LOSS_PER_VIEW 7
#define APG_LOSS_NTERMS 9
#define APG_LOSS_W_TRANS 0
#define APG_LOSS_W_KEYPOINT2D 1
#define APG_LOSS_W_KEYPOINT3D 2
#define APG_LOSS_W_SHAPE 3
#define APG_LOSS_W_ROOTROT 4
#define APG_LOSS_W_POSE 5
#define APG_LOSS_W_BETA 6
#define APG_LOSS_W_CAM 7
#define APG_LOSS_W_LIMBS3D 8
#define APG_LOSS_W_LIMBSTHETA 9
#define APG_LOSS_W_SCALE 10
int64_t apg_loss_workspace_bytes(int B, int V);
int apg_loss_fwd_bwd(int nviews, int cross, int B, int J, int Jg, int V, const float* weights, const void* const* pred,
                     const void* const* gt, float* terms, void* const* grads, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The optimizer step (optim.hip): torch.optim.Adam's update (_single_tensor_adam with maximize = False; L2 weight decay, not the
 * decoupled AdamW form), with or without amsgrad, over a whole list of fp32 tensors in one pass.  Additive under ABI 2: a binding
 * tells a library that has it by looking up apg_adam_step.
 *
 * Per element of tensor i, in place:
 *   g'   = g + weight_decay p
 *   m    = m + (1 - beta1) (g' - m)
 *   v    = beta2 v + (1 - beta2) g'^2
 *   vmax = max(vmax, v)                                                    (amsgrad only, taken after v is updated)
 *   p    = p - (lr / (1 - beta1^step[i])) m / (sqrt(vmax or v) / sqrt(1 - beta2^step[i]) + eps)
 * g is read only.  The host forms lr / (1 - beta1^step[i]) and 1 / sqrt(1 - beta2^step[i]) in double per tensor and rounds each to
 * float once, as it does weight_decay, 1 - beta1, beta2, 1 - beta2 and eps; optim.hip states which products of the sequence are
 * fused.
 *
 *   p, g, m, v, vmax: HOST arrays of ntensors device pointers (like apg_trunk_fwd's params table).  vmax = NULL (the table itself)
 *     selects plain Adam; any other table NULL is APG_EINVAL.
 *   numel, step: HOST arrays of ntensors counts.  step[i] >= 1 is tensor i's step count AFTER this update (torch keeps one per
 *     parameter: a parameter that had no gradient for some steps lags the others).  numel[i] = 0 is accepted and the tensor skipped.
 * The call is stateless: no handle, no workspace, no device-side table, no host synchronisation; the tensors travel in the kernels'
 * argument blocks, 64 per launch, so there are ceil(tensors with elements / 64) launches, each of one workgroup per 4096 elements of
 * each tensor.  Pointers need only 4-byte alignment: a tensor whose pointers are all 16-byte aligned moves in 16-byte accesses, any
 * other in 4-byte accesses, with identical arithmetic -- alignment does not change a bit of any result.  No atomics and no
 * reduction, so results are bit-identical from run to run.
 * Two tensors of one call must not overlap (neither two of its 5 ntensors arrays, nor the same array under two indices).  The
 * library does not check this.
 * APG_EINVAL, before any launch and with nothing written: ntensors < 0, a NULL table other than vmax, a NULL numel or step, a
 * NULL or not 4-byte aligned pointer of a tensor with numel > 0 (a misaligned one also with numel = 0), numel[i] < 0 or above
 * (2^31 - 1) * 4096, step[i] < 1, lr < 0, eps < 0, weight_decay < 0, beta1 or beta2 outside [0, 1) (a NaN fails each of these). */
int apg_adam_step(int ntensors, const void* const* p, const void* const* g, const void* const* m, const void* const* v,
                  const void* const* vmax, const int64_t* numel, const int64_t* step, double lr, double beta1, double beta2, double eps,
                  double weight_decay, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gradient clipping and the non-finite guard (guard/grad_guard.hip): torch.nn.utils.clip_grad_norm_'s global L2 norm and clip coefficient,
 * and a flag for a NaN or Inf gradient, computed on the device in ONE read of the gradients and consumed by the Adam kernel in the
 * same step -- no host copy, no synchronisation, no second pass over the gradients.  Additive under ABI 2: a binding tells a library
 * that has these entries by looking up apg_grad_norm.
 *
 * The guard record, APG_GUARD_BYTES = 16 bytes of device memory, 4-byte aligned, written in full by every apg_grad_norm call:
 *   offset 0   float   coef   (float) min(1, max_norm / (sqrt(S) + 1e-6)): formed in fp64 and rounded once; torch's clip_coef_clamped
 *   offset 4   float   norm   (float) sqrt(S)
 *   offset 8   int32   skip   1 when S is non-finite and skip_nonfinite was set, else 0; when it is 1, coef is written as 1
 *   offset 12  int32          reserved, written as 0
 * S = sum of g^2 over every element of every tensor, accumulated in fp64 from the first add.  The square of a float is exact in fp64,
 * so S cannot overflow for any fp32 gradients (|g| = 1e19 everywhere gives a finite norm), tiny gradients do not flush (|g| = 1e-30
 * gives a non-zero norm), and S is non-finite exactly when some element is NaN or +-Inf: that is what "non-finite" means here.
 * With a non-finite S and skip_nonfinite = 0, coef is written as NaN, so a step that consumes it turns everything it touches into NaN
 * and the failure cannot be overlooked.  (torch's own coefficient is NaN for a NaN norm and 0 for an Inf norm, where 0 * Inf then makes
 * NaN of the offending elements only.)  For a list without any element coef is 1 and norm is 0, whatever max_norm is.
 *
 * apg_grad_norm
 *   g, numel: HOST arrays of ntensors fp32 device pointers and element counts (numel[i] = 0: accepted, the pointer may be NULL).
 *   max_norm >= 0; +inf: guard only (coef = 1 for every finite S).  skip_nonfinite: 0 or not 0.
 *   workspace: at least apg_grad_norm_workspace_bytes(ntensors, numel) bytes (8 per 4096-element chunk and per tensor; negative
 *     for a bad list), 8-byte aligned; the chunk partials and the per-tensor sums.  It carries nothing from call to call and needs no
 *     initialisation.
 *   guard: the record above.  per_tensor: NULL, or ntensors device floats, per_tensor[i] = (float) sqrt(S_i), S_i the tensor's own sum
 *     (0 for a tensor without elements).
 *   counters: NULL, or two device int64 (8-byte aligned) the caller zeroes once: [0] += 1 per call ("seen"), [1] += 1 per call that
 *     set skip ("skipped"); added by one thread of the last launch, stream-ordered, no atomics.
 * Partition and order (apg_adam_step's partition): 4096-element chunks of one tensor, one workgroup of 256 threads each; the tensors
 * travel in the kernels' argument blocks, APG_GRAD_NORM_BATCH = 192 per launch (an empty tensor takes a slot).  Thread t of a chunk
 * owns the float quads at (i * 256 + t) * 4, i = 0 .. 3, moved as one 16-byte access where the tensor's pointer is 16-byte aligned and
 * as four 4-byte accesses otherwise; the last numel mod 4 elements of a tensor are taken one by one by the thread whose quad they
 * start.  An element has the same owner and the same arithmetic on every path.  A thread adds its squares in element order; the 64
 * lanes of a wave are added by the tree l += l + 32, 16, 8, 4, 2, 1; the four waves as ((w0 + w1) + w2) + w3; a second launch adds a
 * tensor's chunks in chunk order (S_i) and a last one the S_i in tensor order (S).  No floating-point atomics, no arrival counter: the
 * order depends on the sizes alone, so norm, coef and per_tensor are bit-identical from run to run and for every alignment.
 * 2 ceil(ntensors / 192) + 1 launches (1 for an empty list: the record is always written), no host synchronisation.
 *
 * apg_grad_scale: g[i][k] = g[i][k] * coef in place for the same table, one correctly rounded product per element, coef read from the
 * guard record on the device.  Where coef == 1 (nothing to clip, or a skipped step) every workgroup returns without a store: the
 * gradients keep their bits, -0 and NaN payloads included.  ceil(ntensors / 192) launches.
 *
 * apg_adam_step_guarded: apg_adam_step with the record.  Every workgroup loads coef and skip.  With skip = 1 it returns before its first
 * store: p, m, v, vmax keep their bits.  Otherwise g2 = coef * g (one correctly rounded product, never fused into what follows) and
 * apg_adam_step's sequence runs on g2; g itself is read only.  With coef = 1 and skip = 0 the result is apg_adam_step's, bit for bit.
 * step[i] is the host's count and advances whether or not the device skips: see FusedAdam (airpose_amd/optim.py).
 *
 * APG_EINVAL, before any launch and with nothing written, the message naming the argument: ntensors < 0, a NULL g table or numel
 * array, numel[i] < 0 or too large, a NULL pointer of a tensor with elements, a pointer that is not 4-byte aligned, max_norm < 0 or
 * NaN, a NULL or misaligned guard, a workspace that is NULL, misaligned or smaller than apg_grad_norm_workspace_bytes says; for
 * apg_adam_step_guarded also every refusal of apg_adam_step. */
#define APG_GUARD_BYTES 16
#define APG_GRAD_NORM_BATCH 192
int64_t apg_grad_norm_workspace_bytes(int ntensors, const int64_t* numel);
int apg_grad_norm(int ntensors, const void* const* g, const int64_t* numel, double max_norm, int skip_nonfinite, void* workspace,
                  int64_t workspace_bytes, void* guard, float* per_tensor, int64_t* counters, void* stream);
int apg_grad_scale(int ntensors, const void* const* g, const int64_t* numel, const void* guard, void* stream);
int apg_adam_step_guarded(int ntensors, const void* const* p, const void* const* g, const void* const* m, const void* const* v,
                          const void* const* vmax, const int64_t* numel, const int64_t* step, double lr, double beta1, double beta2,
                          double eps, double weight_decay, const void* guard, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The real-data fine-tuning loss (loss_real_grad.hip): get_loss of the reference's copenet_real trainers (copenet_twoview.py:100-160,
 * copenet_twoview_sep.py:93-150, hmr.py:82-118, hmr_camswap_difffl.py:92-128, spin.py:86-122) and the gradient of the total with
 * respect to every prediction, in one pass.  2-D keypoints with detector confidences, no 3-D ground truth, a VPoser prior on the body
 * pose.  Additive under ABI 2: a binding tells a library that has it by looking up apg_real_loss_fwd_bwd.
 *
 * With m(x) the mean of x over all its elements, and per view v (summed over the views):
 *   keypoints   m((j2d_v[:, :22] - gt_v[:, :22, :2])^2 conf_v L2)      (B x 22 x 2); conf_v = gt_v[:, :22, 2];
 *               L2 = limbs2d on joints {4, 5, 18, 19}, limbs2d^2 on {7, 8, 20, 21}, 1 elsewhere
 *   vposer      m(z_v^2), z_v = mu + softplus(s) eps_v                  (B x 32); [mu | s] = E(aa_v), aa_v (B x 63) the tgm 0.1.2
 *               axis-angle of rotmat_v[:, 1:22] (the quaternion branches of the zero-padded 3 x 4 form); E below
 *   pose        m((rotmat_0[:, 1:] - rotmat_1[:, 1:])^2)                (B x 21 x 9); with APG_LOSS_CROSS_POSE only
 *   betas       m(betas_v^2) [+ m((betas_0 - betas_1)^2) with APG_LOSS_CROSS_BETAS]      (B x 10)
 *   depth       m(exp(-depth_gain depth_v[:, depth_col])^2)             (B); unweighted, as in the reference
 *   loss        scale * (w_kp keypoints + w_beta betas + w_vposer vposer + w_pose pose + depth)
 * The two-view trainers set APG_LOSS_CROSS_POSE | APG_LOSS_CROSS_BETAS and (depth_col, depth_gain) = (2, 1) on trans; hmr is one
 * view with (0, 10) on its camera, hmr_camswap and spin one view with (2, 1).  The reference's scale is 60.
 *
 * E is VPoser V02_05's encoder_net in eval mode (BatchNorm on running statistics, Dropout the identity), which is two affine maps
 * around one LeakyReLU(0.01): h = W1 aa + b1 (512), [mu | s] = W2 leaky(h) + b2 (64; rows 0 .. 31 mu, 32 .. 63 the logvar head).
 * The caller folds the layers (in fp64) into W1 (512 x 63), b1 (512), W2 (64 x 512), b2 (64), row-major fp32 on the device, and
 * apg_real_loss_pack_encoder lays them out for the kernel in `packed`: apg_real_loss_encoder_bytes() bytes (about 512 KB: each
 * matrix in both orientations, so that the forward and the backward GEMVs both read it coalesced), opaque, valid until overwritten.
 * softplus is torch's (threshold 20).
 *
 *   weights: HOST array of 6 floats, indexed by APG_REAL_LOSS_W_*.
 *   encoder: the packed table (device).
 *   pred: HOST array of APG_REAL_LOSS_PER_VIEW * nviews device pointers; per view rotmat (B x 22 x 3 x 3), betas (B x 10), j2d
 *     (B x J x 2), depth (B x 3: the view's trans or cam).  J >= 22; rows 22 .. J - 1 are never read.  All required.  The two views
 *     may be the same pointers.
 *   gt: HOST array of 2 * nviews device pointers; per view gt (B x Jg x 3: x, y, confidence; Jg >= 22) and eps (B x 32).
 *   terms: 6 device floats, written in the order loss, vposer, pose, keypoints, betas, depth; an absent term is written as 0.
 *   grads: NULL (a forward-only call), or a HOST array of APG_REAL_LOSS_PER_VIEW * nviews device pointers in pred's order and
 *     shapes, each NULL = not needed.  Each given gradient is written in full, not accumulated: rows >= 22 of g_j2d, row 0 of
 *     g_rotmat and the two other columns of g_depth as exact zeros; rows 1 .. 21 of g_rotmat are the pose term's share plus the
 *     vposer term's, which goes back through softplus, E and the axis-angle conversion.  (At an exact identity rotation the
 *     conversion's derivative is the limit 2 daa, where the reference's autograd is NaN.)
 *   workspace: at least apg_real_loss_workspace_bytes(B) bytes (negative for B < 1 or B > 2^30), else APG_ENOMEM; the per-row partial
 *     sums.  It carries nothing from call to call and needs no initialisation.
 * Pointers need only 4-byte alignment; every access is a 4-byte one.  Determinism: no atomics; one workgroup per (view, body) row,
 * every dot product an fmaf chain in index order (the two long ones in four fixed segments added in order), the rows' partials summed
 * per view in index order and a fixed tree -- so terms and gradients are bit-identical from run to run, whatever the alignment and
 * whichever gradients are asked for.  Two launches.
 * APG_EINVAL before any launch, the message naming the argument: a NULL weights, encoder, pred, gt, terms, workspace or table entry
 * of pred / gt, B < 1, J < 22, Jg < 22, nviews outside {1, 2}, cross bits other than APG_LOSS_CROSS_POSE | APG_LOSS_CROSS_BETAS or
 * with nviews = 1, depth_col outside 0 .. 2, and an output (terms, a gradient, the workspace) that overlaps an input. */
#define APG_REAL_LOSS_PER_VIEW 4
#define APG_REAL_LOSS_NTERMS 6
#define APG_REAL_LOSS_W_KEYPOINT2D 0
#define APG_REAL_LOSS_W_BETA 1
#define APG_REAL_LOSS_W_VPOSER 2
#define APG_REAL_LOSS_W_POSE 3
#define APG_REAL_LOSS_W_LIMBS2D 4
#define APG_REAL_LOSS_W_SCALE 5
int64_t apg_real_loss_workspace_bytes(int B);
int64_t apg_real_loss_encoder_bytes(void);
int apg_real_loss_pack_encoder(const float* W1, const float* b1, const float* W2, const float* b2, void* packed, int64_t bytes,
                               void* stream);
int apg_real_loss_fwd_bwd(int nviews, int cross, int B, int J, int Jg, int depth_col, float depth_gain, const float* weights,
                          const void* encoder, const void* const* pred, const void* const* gt, float* terms, void* const* grads,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Evaluation metrics (eval_metrics.hip): what the reference trainers' test_epoch_end computes from the test_step output dicts
 * (copenet_twoview.py:539-601, copenet_singleview.py:394-432, muhmr.py:463-517, hmr.py:365-386): the mean per-joint position error
 * over the 22 body joints (MPJPE), the translation error (MPE) and hmr's angle-axis error, summed into fp64 accumulators that persist
 * across batches.  Additive under ABI 2: a binding tells a library that has it by looking up apg_eval_update.
 *
 * The reference poses SMPL-X four times per batch (ground truth and prediction, two views) with betas = 0 and reads 22 joints of
 * each.  With betas = 0 those joints depend on the 22 rotations and the rest joints J_regressor v_template alone, so no vertex is
 * touched here:
 *   - angle-axis -> matrix is torchgeometry 0.1.2's angle_axis_to_rotation_matrix.  With t2 = r . r and eps = 1e-6: if t2 > eps,
 *     th = sqrt(t2), w = r / (th + eps) (the epsilon stays in the denominator: the axis is deliberately not unit), c = cos th,
 *     s = sin th and
 *       R00 = c + wx^2 (1 - c)       R01 = wx wy (1 - c) - wz s    R02 = wy s + wx wz (1 - c)
 *       R10 = wz s + wx wy (1 - c)   R11 = c + wy^2 (1 - c)        R12 = -wx s + wy wz (1 - c)
 *       R20 = -wy s + wx wz (1 - c)  R21 = wx s + wy wz (1 - c)    R22 = c + wz^2 (1 - c)
 *     otherwise the first-order form I + skew(r), not orthonormal, as tgm leaves it.  (tgm blends the two branches by 0/1 masks and
 *     neither is ever non-finite; the select here is identical.)
 *   - the chain is lbs.batch_rigid_transform restricted to joints 0 .. 21: G_0 = R_0, p_0 = J_0; for j >= 1
 *     G_j = G_parent R_j and p_j = p_parent + G_parent (J_j - J_parent).  parents[j] < j, so the hands and the face never enter.
 *   - joint_err = |p_pred - p_gt|_2 per joint, trans_err = |t_pred - t_gt|_2, angle_err = |a_pred - a_gt|_2 per joint (hmr's metric:
 *     only with APG_EVAL_ANGLE_AXIS and gt angles given).
 *
 * apg_eval_update, one call per batch:
 *   flags: APG_EVAL_ANGLE_AXIS (pred_rot is (B, 22, 3) angle-axis vectors) or APG_EVAL_ROTMAT (pred_rot is (B, 22, 3, 3) matrices).
 *   j_rest: (22, 3) rest joints (device).  parents: HOST array of 22 ints; parents[0] == -1 and 0 <= parents[j] < j.
 *   per_view: HOST array of APG_EVAL_PER_VIEW * views device pointers; per view gt_orient (B, 1, 3, 3), pred_rot, gt_trans (B, 3),
 *     pred_trans (B, 3), gt_angles (B, 22, 3).  The last three may be NULL, the translations only as a pair.
 *   gt_body: (B, 21, 3, 3), shared by the views.
 *   joint_err (views, B, 22), trans_err (views, B), angle_err (views, B, 22): optional per-sample outputs (NULL = not wanted), each
 *     written in full; trans_err / angle_err need the translations / the gt angles of every view.
 *   acc: apg_eval_acc_doubles() = 2 * APG_EVAL_ACC_PER_VIEW doubles (device, 8-byte aligned), ADDED to; the caller zeroes it to start
 *     or reset.  Per view: [0] samples, [1] sum of joint_err, [2 .. 23] the same per joint, [24] sum of trans_err, [25] sum of
 *     angle_err, [26] samples that had a translation, [27] samples that had gt angles.  The second view's block is untouched with
 *     views = 1.  MPJPE = acc[1] / (22 acc[0]), MPE = acc[24] / acc[26], the angle error acc[25] / (22 acc[27]).
 *   workspace: at least apg_eval_workspace_bytes(B, views) bytes (negative for B < 0 or views outside {1, 2}; positive and
 *     non-decreasing in B otherwise), 8-byte aligned, else APG_ENOMEM; the workgroups' partial sums.  It carries nothing from call
 *     to call and needs no initialisation.
 * All other data is fp32, contiguous, 4-byte aligned.  Determinism: no atomics and no arrival counter; each workgroup sums its
 * samples in index order in fp64, a second launch adds the workgroups' partials in index order in fp64 and adds the total to acc.
 * The partition depends on (B, views) alone, so accumulators and per-sample outputs are bit-identical from run to run.  Two
 * launches, no host synchronisation.  B = 0 is a success without a launch: acc is untouched.
 * APG_EINVAL before any GPU call, the message naming the argument: B < 0, views outside {1, 2}, flags neither of the two, a NULL
 * j_rest, parents, per_view, gt_body, acc, workspace, gt_orient or pred_rot, a bad parents table, a pointer that is not 4-byte
 * (acc, workspace: 8-byte) aligned, a translation given by half, gt_angles with APG_EVAL_ROTMAT, trans_err / angle_err asked for
 * without their inputs. */
#define APG_EVAL_ANGLE_AXIS 0
#define APG_EVAL_ROTMAT 1
#define APG_EVAL_PER_VIEW 5
#define APG_EVAL_ACC_PER_VIEW 28
int64_t apg_eval_workspace_bytes(int B, int views);
int64_t apg_eval_acc_doubles(void);
int apg_eval_update(int B, int views, int flags, const float* j_rest, const int* parents, const void* const* per_view,
                    const float* gt_body, float* joint_err, float* trans_err, float* angle_err, double* acc, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh overlay renderer (render.hip): what the reference's utils/renderer.py Renderer draws with pyrender -- n posed meshes over n
 * background images, for summaries() -- stated as ray casting.  Additive under ABI 2: a binding tells a library that has it by
 * looking up apg_render_overlay.  pyrender is absent, so the half-pixel convention and the shading are UNPINNED; the geometry is
 * pinned by this text.
 *
 * Camera coordinates are x right, y down, z forward (the reference's 180 degree turn about x only converts to GL's camera and is
 * absorbed).  A vertex is p = R v + t with the image's R, t.  Pixel (row i, column j) owns the ray
 * d = ((j + 0.5 - cx) / fx, (i + 0.5 - cy) / fy, 1).  For face f = (p0, p1, p2):
 *   w0 = d . (p1 x p2), w1 = d . (p2 x p0), w2 = d . (p0 x p1), det = p0 . (p1 x p2)
 *   the face is drawn iff det < 0 strictly (front-facing for outward counter-clockwise faces; degenerate and repeated-index faces
 *   drop out) and all its vertices are finite; the ray hits it iff -w0, -w1, -w2 >= 0 (inclusive on all three edges: a shared edge
 *   may be claimed twice, never left uncovered) and z = det / (w0 + w1 + w2) has znear <= z <= zfar.
 * The pixel shows the hit with the smallest z and, on exactly equal z, the lowest face index: both are independent of any order, so
 * every output is bit-identical from run to run.
 *   out_depth (n, H, W): that z, 0 where nothing is hit.  out_face (n, H, W) int32: the face, -1 where nothing is hit.  Both optional.
 *   out_rgb (n, 3, H, W): the colour where hit, elsewhere the background's pixel bit for bit (0 with a NULL background).
 * Shading, a stand-in without pyrender's specular lobe: the vertex normal is the normalised sum of (p1 - p0) x (p2 - p0) over the
 * vertex's faces with finite vertices in ascending face order (csr_offsets (V + 1), csr_faces (csr_len <= 3 F): the faces of vertex v are
 * csr_faces[csr_offsets[v] .. csr_offsets[v + 1]), ascending, a face once per distinct vertex; no float atomics).  The normals are
 * interpolated with b_k = w_k / (w0 + w1 + w2), the hit point's barycentrics (perspective-correct), renormalised to n, and
 *   colour = min(1, base_rgb * (ambient + diffuse * max(0, -n_z)));   a zero-length normal gives the ambient term only.
 *
 * apg_render_overlay: vertices (n, V, 3) f32, faces (F, 3) i32, R (n, 3, 3) row-major or NULL = identity, t (n, 3) or NULL = zero,
 * background (n, 3, H, W) f32 or NULL = black; it must not be out_rgb.  All device pointers, contiguous, 4-byte aligned.  Face and
 * CSR entries outside their tables are skipped on the device (such a face is not drawn); the caller should validate them once.
 * workspace: at least apg_render_workspace_bytes(n, H, W, V, F) bytes (negative outside the limits below; non-decreasing in every
 * argument), 16-byte aligned (it holds 16-byte records), else APG_ENOMEM; it carries nothing from call to call and needs no
 * initialisation.
 * Limits: 0 <= n <= 65535; 1 <= H, W <= 16384; 1 <= V, F <= 2^24; n H W, n V and n F at most 2^36.  n = 0 succeeds without a launch.
 * APG_EINVAL before any GPU call, the message naming the argument: a size outside the limits, csr_len outside 0 .. 3 F, a NULL
 * vertices, faces, csr_offsets, csr_faces, out_rgb or workspace, a misaligned pointer (workspace: 16 bytes, the rest 4), fx, fy, znear not positive and finite,
 * cx, cy not finite, zfar < znear, a negative or non-finite base colour, ambient or diffuse, out_rgb == background.
 * Five launches on `stream`, no host synchronisation. */
int64_t apg_render_workspace_bytes(int n, int H, int W, int V, int F);
int apg_render_overlay(int n, int V, int F, int H, int W, const float* vertices, const int* faces, const int* csr_offsets,
                       const int* csr_faces, int csr_len, const float* R, const float* t, float fx, float fy, float cx, float cy,
                       float znear, float zfar, const float* background, float base_r, float base_g, float base_b, float ambient,
                       float diffuse, float* out_rgb, float* out_depth, int* out_face, void* workspace, int64_t workspace_bytes,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh metrics (eval_align.hip): the error between a predicted and a ground-truth point set as it stands, after root alignment and
 * after Procrustes alignment -- MPJPE / PVE, their root-aligned forms and PA-MPJPE / PA-PVE, the numbers mesh-recovery papers
 * tabulate.  The reference computes none of them.  Additive under ABI 2: a binding tells a library that has it by looking up
 * apg_align_update.
 *
 * For a prediction P and a ground truth Q, (B, N, 3) fp32 each, per sample, all sums over the N points:
 *   abs  = mean_i |p_i - q_i|
 *   root = mean_i |(p_i - r_p) - (q_i - r_q)| with the root points r_p, r_q given separately (3 floats per sample each)
 *   pa   = mean_i |s R (p_i - mu_p) + mu_q - q_i| with mu the sets' means and (s, R) the least-squares similarity (Umeyama / Kabsch
 *          with the reflection fix): K = sum (q_i - mu_q)(p_i - mu_p)^T = U S V^T, D = diag(1, 1, sign(det U det V)), R = U D V^T
 *          (det R = +1 always), s = tr(S D) / sum |p_i - mu_p|^2.  If sum |p_i - mu_p|^2 = 0 (N = 1 included): s = 0, R = I and the
 *          error is |mu_q - q_i|.  For collinear points (rank K < 2) the rotation is not unique: the outputs are finite and det R = +1.
 * The moments and the 3 x 3 problem are taken in fp64 about a pivot (point 0 of each set), so a body of 0.5 m extent 10 m from the
 * camera keeps its covariance; each residual is formed in fp64, rounded to float once per component, its norm taken in fp32.
 *
 * apg_align_update, one call per batch and point set:
 *   pred_stride, gt_stride: floats from one sample to the next, at least 3 N (an array may hold more than N points per sample).
 *   per_view: HOST array of APG_ALIGN_PER_VIEW * views device pointers; per view pred, gt, pred_root, gt_root.  The roots may be
 *     NULL, only as a pair: root is then neither computed nor counted for that view.  pred_root_stride, gt_root_stride: floats from
 *     one sample's root to the next, at least 3 (read only where roots are given).
 *   err (views, B, 3): optional per-sample abs, root, pa (root = 0 where no roots are given).  transform (views, B, 13): optional
 *     per-sample s, R row-major (9), t = mu_q - s R mu_p (3), so that s R p + t lies on q.  Each written in full.
 *   acc: apg_align_acc_doubles() = 2 * APG_ALIGN_ACC_PER_VIEW doubles (device, 8-byte aligned), ADDED to; the caller zeroes it to
 *     start or reset.  Per view: [0] samples, [1] sum of abs, [2] sum of root, [3] sum of pa, [4] samples that had roots.  The second
 *     view's block is untouched with views = 1.  The batch means are acc[1] / acc[0], acc[2] / acc[4], acc[3] / acc[0].
 *   workspace: at least apg_align_workspace_bytes(B, views, N) bytes (negative outside the limits below), 8-byte aligned, else
 *     APG_ENOMEM; the samples' means.  It carries nothing from call to call and needs no initialisation.
 * All other data is fp32, 4-byte aligned, a sample's points contiguous.  Limits: 1 <= B <= 2^22, 1 <= N <= 2^24.
 * Determinism: no atomics and no arrival counter; a workgroup owns one (view, sample) and sums in a fixed order in fp64 (thread,
 * wave, workgroup), a second launch adds the samples' means in sample order in fp64 and adds the total to acc.  The partition depends
 * on N alone, so every output is bit-identical from run to run.  Two launches, no host synchronisation.
 * APG_EINVAL before any GPU call, the message naming the argument: B or N outside the limits, views outside {1, 2}, a stride below
 * 3 N (roots: 3), a NULL per_view, pred, gt, acc or workspace, a root given by half, a pointer that is not 4-byte (acc, workspace:
 * 8-byte) aligned. */
#define APG_ALIGN_PER_VIEW 4
#define APG_ALIGN_ACC_PER_VIEW 5
int64_t apg_align_workspace_bytes(int B, int views, int N);
int64_t apg_align_acc_doubles(void);
int apg_align_update(int B, int views, int N, int64_t pred_stride, int64_t gt_stride, int64_t pred_root_stride,
                     int64_t gt_root_stride, const void* const* per_view, float* err, float* transform, double* acc, void* workspace,
                     int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Cross-view metrics (xview_metrics.hip): how well the two views of a calibrated camera pair agree on one body -- what the
 * reference's result scripts print for real footage, which has no 3-D ground truth (copenet_real_res_compile.py:132-143,
 * final_res_compile.py:149-152: each view's prediction carried into the world frame by the inverse extrinsics, the distance between
 * the two; utils/geometry.py:160-192 lstsq_triangulation; the confidence-weighted reprojection term of copenet_twoview.py:112-123).
 * Additive under ABI 2: a binding tells a library that has it by looking up apg_xview_update.
 *
 * Per sample b, with E_v = extr_v[b] = [R_v | t_v] (world -> camera; rows 0 .. 2 of a row-major 3 x 4 or 4 x 4 matrix, row 3 is never
 * read) and W_v(p) = R_v^T (p - t_v), the transpose taken as the inverse:
 *   skip rule: the sample is skipped and counted under `skipped` if an entry of rows 0 .. 2 of either extr is not finite, or if
 *     max |R_v^T R_v - I| > 1e-3 for either view.  The gate is a design constant, not a measurement: an fp32 rotation out of
 *     angle_axis_to_rotation_matrix is orthonormal to about 1e-6, a matrix that misses by 1e-3 is not a rotation and its transpose is
 *     not its inverse.  A skipped sample adds to no other slot, its per-sample row is 1 followed by zeros, its tri rows are zeros.
 *   joint_gap_world  = mean over the first n_joints joints of |W_0(p0_i) - W_1(p1_i)|;  vertex_gap_world the same over the N vertices
 *   joint_gap_root   = the same after subtracting each view's root: |R_0^T (p0_i - r0) - R_1^T (p1_i - r1)|; vertex_gap_root likewise
 *     with the same roots.  The root is a pointer and a stride: the predicted translation, joint 0, or anything else.
 *   trans_gap        = |W_0(s0) - W_1(s1)| of the two translations
 *   orient_gap_deg   = the angle between R_0^T Q0_0 and R_1^T Q1_0 (the root's rotation carried into the world)
 *   pose_gap_deg     = the mean over the body joints j = 1 .. 21 of the angle between Q0_j and Q1_j
 *     angle formula: the angle of A and B is that of D = A^T B, atan2(|(D21 - D12, D02 - D20, D10 - D01)|, tr D - 1), in degrees,
 *     in fp64 -- not acos of the trace, which loses half the digits near 0 and near 180 degrees.  The rotations are (22, 3, 3)
 *     matrices (APG_XVIEW_ROTMAT) or (22, 3) angle-axis vectors (APG_XVIEW_ANGLE_AXIS) taken through tgm 0.1.2's
 *     angle_axis_to_rotation_matrix in fp32, the formula given under the evaluation metrics above.
 *   reproj_px_v      = sum_i c_i |j2d_v,i - k_v,i| / sum_i c_i over the first 22 joints, k = (x, y) and c the confidence of keypoint
 *     row i = (x, y, c); a keypoint counts where x, y, c are finite and c > 0; reproj_n_v is their number.  A sample whose
 *     sum of c is 0 adds to neither the sum nor its count.
 *   triangulation (lstsq_triangulation for two cameras, unweighted, per joint i < 22, in fp64):
 *     n_v = ((x - cx_v) / fx_v, (y - cy_v) / fy_v) with fx = K[0][0], cx = K[0][2], fy = K[1][1], cy = K[1][2] of intr_v[b]; no
 *     other entry is read (the reference's K^-1 agrees where the skew is 0).  Rows n_v[r] E_v[2, :3] - E_v[r, :3], right side
 *     E_v[r, 3] - E_v[2, 3] n_v[r], r = 0, 1: a 4 x 3 system A T = y solved through its normal equations (A^T A) T = A^T y by
 *     cofactors.
 *     validity rule: T_i is valid iff both confidences are > 0, x, y, c of both keypoints and both n_v are finite, the rays
 *     d_v = R_v^T (n_v, 1) have |d_0 x d_1|^2 / (|d_0|^2 |d_1|^2) >= min_sin2, and T_i is finite.
 *     tri_mpjpe_v = mean over the valid joints of |W_v(p_v,i) - T_i|; tri_n is their number.
 * Every point is carried in fp64, a difference is rounded to float once per component and its norm taken in fp32
 * (sqrtf(fmaf(d2, d2, fmaf(d1, d1, d0 * d0)))); sums are fp64.  Two views that hold the same bits under identity extrinsics give
 * every gap exactly 0.
 *
 * apg_xview_update, one call per batch:
 *   views: 2.  n_joints: the joints compared (at least 1).  N: the vertices per sample, 0 = none.
 *   flags: APG_XVIEW_ANGLE_AXIS or APG_XVIEW_ROTMAT, what `rot` holds.
 *   per_view: HOST array of 2 * APG_XVIEW_PER_VIEW device pointers; per view joints (n_joints x 3; 22 x 3 at least with intr), extr,
 *     vertices (N x 3), root (3), trans (3), rot, j2d (22 x 2), keypoints (22 x 3), intr (3 x 3).  All but joints and extr may be
 *     NULL, for both views or neither; vertices exactly when N > 0; j2d needs keypoints, intr needs keypoints, keypoints need one of
 *     the two.  strides: HOST array of APG_XVIEW_PER_VIEW int64: floats from one sample to the next of each entry (the same in both
 *     views), at least the entry's size (extr: 12); read only where the entry is given.
 *   min_sin2: sin^2 of the smallest ray angle a triangulation is accepted at, in 0 .. 1.
 *   per_sample (B, APG_XVIEW_PER_SAMPLE): optional, written in full: [0] skipped (1 / 0), [1] joint_gap_world, [2] joint_gap_root,
 *     [3] vertex_gap_world, [4] vertex_gap_root, [5] trans_gap, [6] orient_gap_deg, [7] pose_gap_deg, [8] [9] reproj_px of view 0 / 1,
 *     [10] [11] reproj_n, [12] [13] tri_mpjpe of view 0 / 1 over the sample's valid joints, [14] tri_n, [15] 0; 0 where not fed.
 *   tri (B, 22, 4): optional (needs intr), written in full: x, y, z, valid (1 / 0) in the world frame; zeros where not valid.
 *   acc: apg_xview_acc_doubles() = APG_XVIEW_ACC doubles (device, 8-byte aligned), ADDED to; the caller zeroes it to start or reset:
 *     [0] samples seen (skipped ones included), [1] skipped, [2] sum of joint_gap_world, [3] sum of joint_gap_root, [4] samples that
 *     had roots, [5] sum of vertex_gap_world, [6] sum of vertex_gap_root, [7] samples that had vertices, [8] samples that had
 *     vertices and roots, [9] sum of trans_gap, [10] samples that had translations, [11] sum of orient_gap_deg, [12] sum of
 *     pose_gap_deg, [13] samples that had rotations, [14] [15] sum of reproj_px of view 0 / 1, [16] [17] samples whose sum of c was
 *     > 0 in view 0 / 1, [18] [19] sum of reproj_n, [20] samples that had j2d, [21] [22] sum over the valid joints of
 *     |W_v(p_v,i) - T_i| of view 0 / 1, [23] tri_n, [24] samples that had intr, [25] reserved, untouched.  All counts but [0] and
 *     [1] leave skipped samples out.  The means: [2] / ([0] - [1]), [3] / [4], [5] / [7], [6] / [8], [9] / [10], [11] / [13],
 *     [12] / [13], [14] / [16], [15] / [17], [21] / [23], [22] / [23].
 *   workspace: at least apg_xview_workspace_bytes(B, 2, N) bytes (negative outside the limits below), 8-byte aligned, else
 *     APG_ENOMEM; the workgroups' partial sums.  It carries nothing from call to call and needs no initialisation.
 * All other data is fp32, 4-byte aligned; every access is a 4-byte one, so alignment changes no bit.
 * Limits: 1 <= B <= 2^22, 1 <= n_joints <= 2^16, 0 <= N <= 2^24, B * ceil(N / 1024) < 2^31.
 * Determinism: no atomics and no arrival counter; a workgroup owns one (sample, chunk of 1024 vertices) and sums in a fixed order in
 * fp64 (thread, wave, workgroup); a second launch adds a sample's chunks in chunk order and the samples in a fixed order in fp64 and
 * adds each total to acc.  The partition depends on (B, N) alone, so every output is bit-identical from run to run.  Two launches,
 * no host synchronisation.
 * APG_EINVAL before any GPU call, the message naming the argument: B, n_joints or N outside the limits, views other than 2, flags
 * neither of the two, min_sin2 outside 0 .. 1, a NULL strides, per_view, joints, extr, acc or workspace, an optional entry given for
 * one view only, vertices without N or N without vertices, j2d or intr without keypoints, keypoints alone, tri without intr, a stride
 * below its entry's size, a pointer that is not 4-byte (acc, workspace: 8-byte) aligned.
 *
 * apg_xview_triangulate: the solve alone, on the same device function.  kp0, kp1 (B, J, 3) = x, y, c; intr0, intr1 (B, 3, 3);
 * extr0, extr1 (B, 4, 4) (rows 0 .. 2 are read); out (B, J, 4) = x, y, z, valid, zeros where not valid -- which includes every joint
 * of a sample the skip rule rejects.  1 <= B <= 2^22, 1 <= J <= 2^16.  One launch. */
#define APG_XVIEW_ANGLE_AXIS 0
#define APG_XVIEW_ROTMAT 1
#define APG_XVIEW_PER_VIEW 9
#define APG_XVIEW_ACC 26
#define APG_XVIEW_PER_SAMPLE 16
int64_t apg_xview_workspace_bytes(int B, int views, int N);
int64_t apg_xview_acc_doubles(void);
int apg_xview_update(int B, int views, int n_joints, int N, int flags, const int64_t* strides, const void* const* per_view,
                     double min_sin2, float* per_sample, float* tri, double* acc, void* workspace, int64_t workspace_bytes,
                     void* stream);
int apg_xview_triangulate(int B, int J, const float* kp0, const float* kp1, const float* intr0, const float* intr1,
                          const float* extr0, const float* extr1, double min_sin2, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * AirPose+ on a whole sequence (seq_fit.hip): the per-frame work on either side of the fitting loop (ap_fit_run of
 * libairpose_hip.so) -- the loop's initial state and filtered detections from the network's outputs (bundle_adj.py:176-200,
 * copenet_real.py:105-106) and the fitted bodies under the names the rest of the package reads (bundle_adj.py:404-412, 510-516).
 * Additive under ABI 2: a binding tells a library that has it by looking up apg_seq_init.  Two stateless entry points, no workspace;
 * all pointers are device pointers to contiguous fp32 (robust: int32), 4-byte aligned unless stated.  1 <= L <= 2^22.
 *
 * apg_seq_init, per frame l:
 *   angles0, angles1 (L, 22, 3): axis-angle, joint 0 the root.  trans0, trans1 (L, 3).
 *   det (2 views, L, 2 detectors, 24, 3) = x, y, confidence; detector 0 is OpenPose, detector 1 AlphaPose.
 *   W1 (512, 63), b1 (512), Wmu (32, 512; 16-byte aligned), bmu (32): VPoser's encoder in eval mode folded into two affine maps
 *     (mu rows only).
 *   z (L, 32)      = Wmu leaky_0.01(W1 angles0[l, 1:22] + b1) + bmu: the posterior mean of view 0's body pose.
 *   phi (2, L, 6)  = the first two ROWS of R(angles_v[l, 0]), row-major (pytorch3d matrix_to_rotation_6d), with R pytorch3d 0.3.0's
 *     axis_angle_to_matrix: q = (cos(t / 2), r sin(t / 2) / t), t = |r|, sin(t / 2) / t replaced by 1/2 - t^2 / 48 for t < 1e-6,
 *     then quaternion_to_matrix with two_s = 2 / |q|^2.  r = 0 gives the identity exactly.
 *   tau (2, L, 3)  = trans_v, bit for bit.
 *   j2d (2, L, 2, 24, 3) = det with the confidence of BOTH detectors set to 0 where sqrt(dx^2 + dy^2) > agreement_px between the two
 *     detectors' positions of that view, frame and joint (strict); x and y bit for bit.  j2d must not be det.
 *   robust (L) int32 = 1 iff the filtered AlphaPose confidences, added in the order view 0 joint 0 .. 23, view 1 joint 0 .. 23 in
 *     fp32, are > robust_conf (strict), else 0.
 * apg_seq_export, per frame l:
 *   z (L, 32), phi (2, L, 6), tau (2, L, 3) as the fitter returns them; w1 (512, 32), b1, w2 (512, 512), b2, w3 (126, 512), b3: the
 *     VPoser decoder's Linear layers as torch stores them (w1, w2, w3: 16-byte aligned).
 *   thetas (L, 63)          = decode(z)["pose_body"]: the MLP (LeakyReLU 0.01), Gram-Schmidt on the (21, 3, 2) reshape, tgm 0.1.2's
 *     rotation_matrix_to_angle_axis -- the formulae of the fitter's own decoder.
 *   root_rot (2, L, 3, 3)   = pytorch3d rotation_6d_to_matrix(phi): rows b1, b2, b1 x b2.
 *   smpl_wrt_cam (2, L, 4, 4) = [root_rot | tau; 0 0 0 1].
 *   cam1_wrt_cam0 (L, 4, 4) = smpl_wrt_cam0 smpl_wrt_cam1^-1, the inverse formed as the rigid [R^T | -R^T t].
 * APG_SEQ_ROWS frames share a workgroup; every sum has a fixed order and there is no atomic, so every output is bit-identical from
 * run to run.  One launch each on `stream`, no host synchronisation.
 * APG_EINVAL before any GPU call, the message naming the argument: L outside the limits, a NULL or misaligned pointer,
 * agreement_px negative or not finite, robust_conf not finite, j2d == det. */
#define APG_SEQ_ROWS 4
int apg_seq_init(int L, const float* angles0, const float* angles1, const float* trans0, const float* trans1, const float* det,
                 const float* W1, const float* b1, const float* Wmu, const float* bmu, float agreement_px, float robust_conf, float* z,
                 float* phi, float* tau, float* j2d, int* robust, void* stream);
int apg_seq_export(int L, const float* z, const float* phi, const float* tau, const float* w1, const float* b1, const float* w2,
                   const float* b2, const float* w3, const float* b3, float* thetas, float* root_rot, float* smpl_wrt_cam,
                   float* cam1_wrt_cam0, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Real-data batches (seq_batch.hip): what copenet_real.__getitem__ (copenet_real/dsets/copenet_real.py:162-258) and the agreement
 * filter of its __init__ (:105-106) compute between the raw detections and the network's inputs, for frames [a, a + n) of an
 * L-frame sequence and both views, in ONE launch: the filtered detections, the crop box round the surviving OpenPose keypoints, bb,
 * and the keypoints in crop coordinates.  The boxes stay on the device: ap_preprocess_crops (libairpose_hip.so) reads `crops` as it
 * is, and nobody validates them on the host, so THE KERNEL guarantees the box invariant below for any bit pattern in det.
 * Additive under ABI 2: a binding tells a library that has it by looking up apg_real_batch.  Stateless, no workspace; all pointers are
 * device pointers to contiguous arrays, 4-byte aligned; size and principal are HOST arrays read during the call.
 *
 *   det (2 views, L, 2 detectors, 24, 3) fp32 = x, y, confidence, as apg_seq_init takes it; detector 0 is OpenPose, detector 1 AlphaPose.
 *   principal: HOST (2, 2) = cx, cy per view (K[0, 2], K[1, 2]), > 0 and finite.  size: HOST (2, 2) int = H_v, W_v per view, >= 1.
 *   agreement_px >= 0 and finite (the reference: 100); border: whole pixels, 0 .. 2^20 (the reference: 50).
 * per (view v, frame a + i), i < n -- every output is written for every (v, i):
 *   j2d (2, n, 2, 24, 3)      = det with the confidence of BOTH detectors set to 0 where sqrt(dx^2 + dy^2) > agreement_px (strict); x and
 *     y bit for bit.  The same arithmetic as apg_seq_init: for the same frames the two j2d are bit-equal.
 *   crops (2, n, 4) int32     = y0, y1, x0, x1, the layout ap_preprocess_crops reads; crop_info (2, n, 2, 2) int32 = [[y0, x0], [y1, x1]].
 *     From the filtered OpenPose keypoints with confidence != 0: x0 = max(trunc(min x - border), 0), x1 = min(trunc(max x + border), W),
 *     y likewise with H; trunc is Python's int(), towards zero, never to nearest (where the clamps leave its operand
 *     it is >= 0, so floor says the same; min x - border < 0 gives 0 through the clamp).  The sums are formed in fp64, as the
 *     reference forms them, so they are exact for every fp32 x.  With no such keypoint the set is {0} on both axes (the reference's fallback).
 *   bb (2, n, 3)              = ((x0 + x1) / 2 / cx - 1, (y0 + y1) / 2 / cy - 1, scale), each operation rounded to fp32 in that order
 *     (no fused multiply-add); scale = (float)(224.0 / (double)max(y1 - y0, x1 - x0)), the expression of ap_preprocess_crops: the
 *     two scales are bit-equal.
 *   j2d_crop (2, n, 2, 24, 3) = for both detectors xy' = scale * (xy - (bb_xy + 1) * c), confidence copied (the filtered one); each
 *     operation rounded to fp32, no pad offset (the reference applies none).
 *   status (2, n) int32: bit 0 (APG_BATCH_FALLBACK) no keypoint was used, the fallback box was taken; bit 1 (APG_BATCH_CLAMPED) at
 *     least one otherwise usable keypoint was non-finite or outside [0, W] x [0, H]; bit 2 (APG_BATCH_WIDENED) the box was empty
 *     along an axis and was widened to one pixel.
 * The box invariant, for ANY det: 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H.  Three rules give it, each the identity wherever the
 * reference itself works: a keypoint with a non-finite x or y is treated as absent; a finite keypoint outside the frame is clamped
 * to [0, W] x [0, H] before the minimum and maximum are taken; an axis left with x1 <= x0 (border = 0 on one point, a fallback box
 * with border = 0) becomes the one pixel [min(x0, W - 1), min(x0, W - 1) + 1).
 * One wave64 per (view, frame), APG_BATCH_WAVES waves per workgroup, no LDS, no atomic: bit-identical from run to run.  One launch
 * on `stream`, no host synchronisation.
 * APG_EINVAL before any GPU call, the message naming the argument: a NULL or misaligned pointer, L outside 1 .. 2^22, n < 1, a < 0, a + n > L, a
 * frame size < 1 or > 2^20, a principal point not positive and finite, agreement_px negative or not finite, border outside 0 .. 2^20, j2d == det. */
#define APG_BATCH_WAVES 4
#define APG_BATCH_FALLBACK 1
#define APG_BATCH_CLAMPED 2
#define APG_BATCH_WIDENED 4
int apg_real_batch(int L, int a, int n, const float* det, const float* principal, const int* size, float agreement_px, int border,
                  float* j2d, int* crops, int* crop_info, float* bb, float* j2d_crop, int* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Synthetic-data batches (synth_batch.hip): what aerialpeople_crop.__getitem__ (copenet/src/copenet/dsets/aerialpeople.py:81-226)
 * computes between a sample's pickled record and the batch dict, for n samples and both cameras, apart from the file reading and the
 * SMPL-X forward of the canonical body (:179-197, which airpose_amd.SyntheticBatches runs on the existing ap_smplx_fwd).
 * apg_synth_batch: the jittered crop box of each camera (:98-135), bb, the ground truth in each camera's frame (:148-177 with
 * transform_smpl, utils.py:237-256, and perspective_projection with R = I, t = 0), smplpose_rotmat (lbs.batch_rodrigues, epsilon
 * 1e-8) and the per-sample camera shuffle (:208-211).  It reads no image.  apg_synth_crops: the images, from the boxes and the flips
 * that apg_synth_batch left on the device.  Nobody validates a box on the host, so THE KERNEL guarantees the box invariant below for
 * any bit pattern in bb_in.  Additive under ABI 2: a binding tells a library that has them by looking up apg_synth_batch.
 * Stateless, no workspace; all pointers are device pointers to contiguous arrays, 4-byte aligned (frames: any alignment).
 *
 * apg_synth_batch, inputs (c = camera 0 / 1, i < n):
 *   n in 1 .. 65535; V in 1 .. 2^24 vertices; J in 1 .. 2^16 joints; H, W: the frame's size, 1 .. 2^20; Hc, Wc: the canvas's size
 *   (the images apg_synth_crops will read), 1 .. 2^20; margin: whole pixels, 0 .. 2^20 (the reference: 200).
 *   origin: APG_SYNTH_ORIGIN_REGION (0) the canvas holds the region [ymin:ymax, xmin:xmax] of the frame at its top-left (the
 *     reference's pre-cropped dataset), APG_SYNTH_ORIGIN_FRAME (1) the canvas is the whole frame.
 *   jitter, shuffle: 0 or 1; 0 sets the four offsets / the flip to 0.  fx, fy: the focal length (the reference: 1475), finite.
 *   seed, epoch: see the draws.  index (n) int32: the samples' dataset indices.
 *   bb_in (n, 2, 2, 2) int32 = [[x0, y0], [x1, y1]] per camera; intr (n, 2, 3, 3); extr (n, 2, 4, 4) (rows 0 .. 2 are [R | t]);
 *   pose (n, 63) axis-angle; verts (n, V, 3), joints (n, J, 3), orient (n, 3, 3), trans (n, 3): the *_wrt_origin fields; all fp32.
 * The box, per (i, c) and per axis (y with H and Hc, x with W and Wc), in 32-bit integers that cannot overflow:
 *   y0, y1 are clamped to [0, H] (rule 1).
 *   ymin = y0 - margin if y0 - margin > 0 else 0;  ymax = y1 + margin if y1 + margin < H else H  (both comparisons strict).
 *   The draws: Philox4x32-10 (Random123's constants), key = (seed's low word, seed's high word), counter = (index[i], epoch, c, 0).
 *     Its words 0 .. 3 give the offsets in the reference's draw order -- ymin side, ymax side, xmin side, xmax side -- over the
 *     ranges r = y0 - ymin, ymax - y1, x0 - xmin, xmax - x1: offset = 0 if r == 0 else mulhi32(word, r), which is in [0, r).
 *     flip[i] = bit 31 of word 0 of the counter (index[i], epoch, 2, 0).  A draw depends on (seed, epoch, index, camera) alone.
 *   The crop is [ymin + o0, ymax - o1); if that is empty it becomes the one pixel [min(ymin + o0, H - 1), + 1) (rule 2).
 *   crop_info = [[ymin, xmin], [ymax, xmax]]: the region, as in the reference, NOT the crop.
 *   Canvas coordinates are the crop minus ymin (origin region) or minus 0 (origin frame); if they leave [0, Hc] they are clamped
 *     to 0 <= y0' <= Hc - 1, y0' + 1 <= y1' <= Hc (rule 3).  `crops` holds them; bb and scale are taken from the same box, moved back.
 * The box invariant, for ANY bb_in: 0 <= y0' < y1' <= Hc and 0 <= x0' < x1' <= Wc.  Each rule is the identity wherever the
 * reference itself works (a box inside the frame, a crop that is not empty, a canvas that holds the region or the frame).
 * Outputs, every element written, indexed by SUFFIX s: suffix s of sample i is camera flip[i] ^ s.
 *   crops (2, n, 4) int32 = y0', y1', x0', x1' (canvas, the layout ap_preprocess_crops reads); crop_info (2, n, 2, 2) int32;
 *   status (2, n) int32: bit 0 (APG_SYNTH_CLAMPED) rule 1 moved a corner, bit 1 (APG_SYNTH_WIDENED) rule 2, bit 2
 *     (APG_SYNTH_OUTSIDE) rule 3;  flip (n) int32 = 0 or 1.
 *   bb (2, n, 3) = ((xa + xb) / 2 / cx - 1, (ya + yb) / 2 / cy - 1, scale): xa, xb, ya, yb the box in FRAME coordinates, cx =
 *     intr[i, c, 0, 2], cy = intr[i, c, 1, 2], each operation rounded to fp32 in that order; scale = (float)(224.0 / (double)max(h, w)),
 *     the expression of ap_preprocess_crops and apg_synth_crops: the scales are bit-equal.
 *   intr_out (2, n, 3, 3), extr_out (2, n, 4, 4): copies.
 *   verts_rel (2, n, V, 3), joints_rel (2, n, J, 3) = R p + t evaluated as ((R0 x + R1 y) + R2 z) + t, every product and sum
 *     rounded to fp32 once (no fused multiply-add); each vertex is read once and written for both cameras.
 *   orient_rel (2, n, 3, 3) = R orient and trans_rel (2, n, 3) = R trans + t, sums in the same order.
 *   j2d (2, n, J, 2) = (fx (x / z) + cx, fy (y / z) + cy) of joints_rel; j2d_crop (2, n, J, 2) = scale * (j2d - (bb_xy + 1) * c),
 *     no pad offset (the reference applies none); each operation rounded to fp32.
 *   pose_rotmat (n, 21, 3, 3) = I + sin(a) K + (1 - cos(a)) K K, a = |r + 1e-8|, K the cross-product matrix of r / a, K K summed
 *     in bmm's order.
 * Two launches on `stream` (the per-sample records and joints; the vertices), no LDS traffic between samples, no atomic, every sum
 * in a fixed order: bit-identical from run to run.  No host synchronisation.
 *
 * apg_synth_crops: one launch over (pixel, sample, suffix).  frames (2 cameras, n, Hc, Wc, 3) uint8; bgr as ap_preprocess_crops;
 *   crops (2, n, 4) and flip (n) as apg_synth_batch wrote them.  For suffix s of sample i it reads the canvas of camera
 *   (flip[i] & 1) ^ s through crops[s, i] and writes im (2, n, 3, 224, 224), scale (2, n), pad (2, n, 2) int32 = left, top.  The
 *   per-pixel arithmetic is ONE source with ap_preprocess_crops (csrc/preprocess_px.inc): the same bits for the same box.  A row
 *   whose box breaks the invariant is neither read through nor written (apg_synth_batch writes no such box).
 * APG_EINVAL before any GPU call, the message naming the argument: a NULL or misaligned pointer, a size outside its limits, origin,
 * jitter, shuffle or bgr outside their values, fx or fy not finite, an output that is its own input. */
#define APG_SYNTH_ORIGIN_REGION 0
#define APG_SYNTH_ORIGIN_FRAME 1
#define APG_SYNTH_CLAMPED 1
#define APG_SYNTH_WIDENED 2
#define APG_SYNTH_OUTSIDE 4
#define APG_SYNTH_THREADS 128
int apg_synth_batch(int n, int V, int J, int H, int W, int Hc, int Wc, int margin, int origin, int jitter, int shuffle, float fx,
                    float fy, uint64_t seed, int epoch, const int* index, const int* bb_in, const float* intr, const float* extr,
                    const float* pose, const float* verts, const float* joints, const float* orient, const float* trans, int* crops,
                    int* crop_info, int* status, int* flip, float* bb, float* intr_out, float* extr_out, float* verts_rel,
                    float* joints_rel, float* orient_rel, float* trans_rel, float* j2d, float* j2d_crop, float* pose_rotmat,
                    void* stream);
int apg_synth_crops(int n, int Hc, int Wc, int bgr, const unsigned char* frames, const int* crops, const int* flip, float* im,
                    float* scale, int* pad, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Crop augmentation (augment.hip): blur, colour, gamma, noise and occluders on the (2, n, 3, 224, 224) crops that apg_synth_crops and
 * ap_preprocess_crops write, without leaving the device.  The reference's dataset lists its augmentations, commented out, at
 * copenet/src/copenet/dsets/aerialpeople.py:72-76 (imgaug: brightness, hue and saturation, colour temperature, per-channel gamma,
 * grayscale); parity with imgaug is UNPINNED -- THIS TEXT is the contract.  apg_augment_draw writes a parameter set from stateless
 * draws; apg_augment_crops applies a parameter set (drawn or planted) in ONE launch for both views and all n images, the image read
 * once and written once.  Additive under ABI 2: a binding tells a library that has them by looking up apg_augment_crops.  Stateless,
 * no workspace; all pointers are device pointers to contiguous arrays, 4-byte aligned, except cfg, a HOST array.
 *
 * The parameter set, per (suffix s, sample i):
 *   blur_taps (2, n, 7) fp32: the half kernel w0 .. w6 of a normalised, symmetric, separable blur.  The radius r is the index of the
 *     last non-zero tap; r = 0 skips the stage (w0 is then not read).
 *   color (2, n, 3, 4) fp32 = [M | b], row-major.  Exactly [I | 0] skips the stage.
 *   gamma (2, n, 3) fp32, per channel; exactly 1 skips that channel.
 *   noise_sigma (2, n) fp32; 0 skips the stage.
 *   rects (2, n, 4, 4) int32 = y0, y1, x0, x1 in crop pixels (rows and columns of the 224 x 224 image); y1 <= y0 or x1 <= x0: empty.
 *   rect_rgb (2, n, 4, 3) fp32: the fill colours, clamped to [0, 1] when they are used.
 *
 * apg_augment_crops, per image, on de-normalised RGB v = x * std + mean (mean 0.485, 0.456, 0.406, std 0.229, 0.224, 0.225), every
 * product, sum and quotient below rounded to fp32 once, in the order written (no fused multiply-add); clamp(t) = min(max(t, 0), 1):
 *   The content rectangle is recomputed from crops (2, n, 4) int32 = y0, y1, x0, x1 exactly as preprocess_px.inc computes it: h = y1 -
 *     y0, w = x1 - x0, scale = 224.0 / (double)max(h, w), dw = (int)(scale * w), dh = (int)(scale * h), top = (224 - dh) / 2, left =
 *     (224 - dw) / 2: rows top .. top + dh - 1, columns left .. left + dw - 1.  Every other pixel is padding.
 *   Padding pixels are copied bit for bit, always.  With dw == 0 or dh == 0, or a box with y1 <= y0 or x1 <= x0 (APG_AUG_BAD_BOX), the
 *     whole image is copied.  An image whose stages are all skipped is copied bit for bit: no de-normalise / re-normalise round trip.
 *   0. v = x * std + mean.
 *   1. Blur (r > 0): a horizontal pass, then a vertical pass over its result; each pass t = w_r p(-r), then t = t + w_|k| p(k) for k =
 *      -r + 1 .. r in that order, p(k) the pixel k columns (rows) away with its coordinate clamped to the content rectangle, so
 *      that padding never bleeds in.
 *   2. Colour (not [I | 0]): v'_c = clamp(((M_c0 v_0 + M_c1 v_1) + M_c2 v_2) + b_c).
 *   3. Gamma (gamma_c != 1): v_c = powf(clamp(v_c), gamma_c); the clamp keeps a de-normalised -1e-8 from becoming a NaN.
 *   4. Noise (sigma != 0): v_c = clamp(v_c + sigma * z_c).  ONE Philox4x32-10 call per pixel, key = (seed's low word, seed's high
 *      word), counter = (index[i], epoch, camera, 0x80000000 | (row * 224 + column)); words (0, 1) and (2, 3) go through Box-Muller with
 *      u1 = ((w >> 8) + 1) * 2^-24 of the first word and u2 = (w >> 8) * 2^-24 of the second: rho = sqrtf(-2 * logf(u1)), phi =
 *      6.2831855f * u2, (rho * cosf(phi), rho * sinf(phi)); z_R, z_G = the pair of words (0, 1), z_B = the cosine of words (2, 3).
 *   5. Occluders: rects 0 .. 3 in that order (a later one covers an earlier one); a pixel of the content rectangle inside rect k
 *      takes clamp(rect_rgb[k]).  A rect reaching outside the content rectangle is clipped to it (APG_AUG_RECT_CLIPPED).
 *   6. out = (v - mean) / std.
 *   The camera of (s, i) is (cam[i] & 1) ^ s with cam (n) int32 on the device (SyntheticBatches' cam0), or cam_all ^ s when cam is
 *     NULL (cam_all = 0 or 1: RealSequenceBatches' first_cam).  index (n) int32: the samples' dataset indices.
 *   Values checked on the device, each reported in status (2, n) int32 and treated as NEUTRAL (APG_AUG_NONFINITE): a non-finite tap
 *     (r = 0), a non-finite entry of color ([I | 0]), a gamma that is non-finite or negative (1), a non-finite noise_sigma (0), a
 *     non-finite rect_rgb (that rect is empty).  With the 7 taps the radius cannot pass APG_AUG_MAX_RADIUS.
 *   One workgroup of APG_AUG_THREADS threads per APG_AUG_TILE x APG_AUG_TILE tile; with r > 0 the tile and its halo of r are staged
 *     de-normalised in LDS and every later stage runs while the pixel is in registers.  A thread's own four pixels move as 16-byte
 *     loads and stores where im and out are 16-byte aligned, as 4-byte ones otherwise; the halo is staged with 4-byte loads.  out must not overlap im: a blur in place would race across tile seams.
 *
 * apg_augment_draw: one launch, one thread per (s, i), writes the whole parameter set and status.  Philox4x32-10, the key as above,
 * counter = (index[i], epoch, camera, k) with k >= 1; apg_synth_batch's jitter and flip use k = 0 and the noise k >= 2^31, so no two
 * streams collide under one seed.  A uniform draw is u = (word >> 8) * 2^-24, exact in fp32; "lo .. hi" below is lo + u * (hi - lo),
 * each operation rounded to fp32.  A gate is on when u < p.  cfg is a HOST array of APG_AUG_CFG floats, all finite:
 *     0 p | 1, 2 blur sigma | 3 brightness B | 4 hue H (degrees) | 5, 6 saturation | 7, 8 channel gain | 9, 10 gamma | 11, 12 grayscale
 *     | 13, 14 noise sigma | 15 occluders (0 .. 4) | 16, 17 occluder side (fractions of 224).
 *   A stage whose range is neutral (sigma 0 .. 0, B = 0, H = 0, 1 .. 1 for saturation, gain and gamma, 0 .. 0 for grayscale and noise,
 *   0 occluders) is off: it leaves its exact neutral value whatever its gate.  Word w of block k:
 *     k = 1: gate blur, sigma, gate brightness, beta = -B .. B          k = 2: gate hue, theta = -H .. H, gate saturation, s
 *     k = 3: gate gain, gain R, G, B                                    k = 4: gate gamma, gamma R, G, B
 *     k = 5: gate grayscale, alpha, gate noise, sigma                   k = 6: gate occluders
 *     k = 7 + j: rect j: side along y, side along x, centre y, centre x k = 11 + j: rect j's colour R, G, B (u itself)
 *   blur_taps: in fp64, r = min(ceil(3 sigma), 6) (APG_AUG_BLUR_CLAMPED where the minimum acts), w_k = exp(-k^2 / (2 sigma^2)) / (w_0
 *     + 2 sum w_k), k <= r, rounded to fp32 once; sigma <= 0 gives 1, 0, ..
 *   color: M composed in fp64 and rounded once: M = diag(gain); M = Hue(theta) M; M = ((1 - s) L + s I) M; M = (alpha L + (1 - alpha) I) M,
 *     each only where its gate is on, L the matrix whose rows are (0.299, 0.587, 0.114).  Hue(theta) = L + cos(theta) (I - L) +
 *     sin(theta) K is the rotation of the I-Q plane of YIQ, K = ((0.168, 0.330, -0.497), (-0.328, 0.035, 0.292), (1.25, -1.05, -0.203)).
 *     b = (beta, beta, beta).  All gates off leaves exactly [I | 0].
 *   rects: for j < occluders, sides hy = (int)(f_y * 224), hx = (int)(f_x * 224) with f = lo .. hi, centres cy = (int)(u * 224), cx
 *     likewise: y0 = cy - hy / 2, y1 = y0 + hy, x0 = cx - hx / 2, x1 = x0 + hx (crop pixels, not clipped here); the others 0, 0, 0, 0.
 * A draw depends on (seed, index, epoch, camera) and cfg alone: not on the batch, the row or the camera shuffle.
 * APG_EINVAL before any GPU call, the message naming the argument: n outside 1 .. 65535, a NULL or misaligned pointer (cam may be
 * NULL), cam_all outside 0 .. 1, a cfg entry that is not finite or outside its range, out overlapping im. */
#define APG_AUG_TILE 32
#define APG_AUG_THREADS 256
#define APG_AUG_MAX_RADIUS 6
#define APG_AUG_MAX_RECTS 4
#define APG_AUG_CFG 18
#define APG_AUG_BLUR_CLAMPED 1
#define APG_AUG_NONFINITE 2
#define APG_AUG_RECT_CLIPPED 4
#define APG_AUG_BAD_BOX 8
int apg_augment_draw(int n, uint64_t seed, int epoch, const int* index, const int* cam, int cam_all, const float* cfg,
                     float* blur_taps, float* color, float* gamma, float* noise_sigma, int* rects, float* rect_rgb, int* status, void* stream);
int apg_augment_crops(int n, uint64_t seed, int epoch, const int* index, const int* cam, int cam_all, const float* im,
                      const int* crops, const float* blur_taps, const float* color, const float* gamma, const float* noise_sigma, const int* rects,
                      const float* rect_rgb, float* out, int* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Camera roll (roll.hip): the geometric augmentation of the training chain, a ROLL OF THE CAMERA ABOUT ITS OPTICAL AXIS by an angle
 * theta, applied to the crops and to every label of a SyntheticBatches / RealSequenceBatches dict without leaving the device.  It is a
 * rigid motion of the camera, so no label becomes approximate and the two views stay consistent through extr.  The reference has
 * no image-plane augmentation: its rottrans_tfm (not called) moves the WORLD frame -- extr and the *_wrt_origin labels -- and no pixel.
 * Flips (a mirrored body is no rigid motion) and zoom (it changes the depth to predict at a fixed focal length) are not built.
 * THIS TEXT is the contract.  Additive under ABI 2: a binding tells a library that has them by looking up apg_roll_crops.  Stateless,
 * no workspace; three launches on `stream` (one per entry), no host copy, no synchronisation; all pointers are device pointers to
 * contiguous arrays, 4-byte aligned (the canvases: any alignment).  Compiled with -ffp-contract=off: outside apg_roll_draw's cos and sin every operation below is ONE
 * fp32 rounding of + - * / in the written order (parentheses are the order), no fused multiply-add, so that a numpy float32
 * restatement gives the same bits.
 *
 * Per sample i < n and suffix s the camera is (cam[i] & 1) ^ s with cam (n) int32 on the device (SyntheticBatches' cam0), or
 * cam_all ^ s when cam is NULL (cam_all = 0 or 1: RealSequenceBatches' cam).  rot (2, n, 2) = (c, sn) = (cos theta, sin theta), drawn
 * or planted; it is not normalised.  From intr (2, n, 3, 3), indexed by suffix: fx = K[0][0], fy = K[1][1], cx = K[0][2], cy =
 * K[1][2], tx = sn * (fx / fy), ty = sn * (fy / fx), and
 *     A(theta)  (x, y) = ((c * x) - (tx * y), (ty * x) + (c * y))        (R2(theta) when fx = fy)
 *     A(-theta) (x, y) = ((c * x) + (tx * y), (c * y) - (ty * x))
 *     Rz(theta) (x, y) = ((c * x) - (sn * y), (sn * x) + (c * y)).
 * Pixel-index coordinates are the projection's coordinates, as the reference treats them.
 *
 * apg_roll_labels, per (s, i):
 *   The decision.  A row whose (c, sn) is exactly (1, 0) is un-rolled and is not tested; its tx and ty are exactly 0 whatever intr
 *     holds (a zero focal length cannot make its OFF_CANVAS corners NaN).  Otherwise (u, v) = A(theta) (bb_x * cx,
 *     bb_y * cy), bb'_x = u / cx, bb'_y = v / cy: the crop box's centre turned about the principal point.  The refusal rule: unless
 *     |bb'_x| <= 1 and |bb'_y| <= 1 (a NaN fails it too) the crop centre would leave a frame centred on the principal point, the
 *     (sample, view) is left un-rolled, (c, sn) := (1, 0) exactly, and APG_ROLL_CENTRE_OUT is set.
 *   rot_used (2, n, 2) = the (c, sn) in force; bb_out (2, n, 3) = (bb'_x, bb'_y, bb_2); status (2, n) int32.
 *   An un-rolled row COPIES bb and every label bit for bit.  A rolled row:
 *     verts (2, n, V, 3), joints (2, n, J, 3), trans (2, n, 3): (x', y') = Rz(theta) (x, y), z copied;
 *     orient (2, n, 3, 3) = Rz R: per column, rows 0 and 1 mixed by Rz(theta), row 2 copied;
 *     extr (2, n, 4, 4): per column (the translation column included), rows 0 and 1 mixed by Rz(theta), rows 2 and 3 copied;
 *     j2d (2, n, P, pstride): (d_x, d_y) = (x - cx, y - cy), p' = (cx + a_x, cy + a_y) with a = A(theta) d;
 *     j2d_crop (2, n, P, pstride): A(theta) applied to the vector itself (it is measured from the crop centre);
 *     with pstride = 3 the third column (the real dict's confidence) is copied bit for bit.
 *   A label pointer that is NULL means the dict has no such key: nothing is read or written for it and its count is not looked at.
 *   crops (2, n, 4) int32 = y0, y1, x0, x1 on the camera's canvas, NOT changed: it keeps describing the un-rolled box, whose height
 *     and width are what apg_augment_crops reads.  scale, pad, crop_info and intr are not touched either.
 *   APG_ROLL_OFF_CANVAS, the "black wedge" signal: with hw = w * 0.5, hh = h * 0.5 (w = x1 - x0, h = y1 - y0) and the centre m =
 *     (x0 + hw, y0 + hh), a corner is q = m + A(-theta) (+-hw, +-hh); the bit is set unless all four have 0 <= q_x <= Wc and
 *     0 <= q_y <= Hc, the size of the camera's canvas.  Status words are written with plain vector stores by one thread per (s, i).
 *   One thread per item (a vertex, a joint, a point, a column): every label byte is read once and written once.  An output must
 *   not overlap its input.
 *
 * apg_roll_crops: im (2, n, 3, 224, 224) from the cameras' canvases, frames0 (n, Hc0, Wc0, 3) and frames1 (n, Hc1, Wc1, 3) uint8,
 * both indexed by CAMERA (SyntheticBatches' one (2, n, Hc, Wc, 3) tensor is frames0 and frames0 + n Hc Wc 3 with equal sizes;
 * RealSequenceBatches' frames0 / frames1 as they are); bgr as ap_preprocess_crops; crops as above; rot_used as apg_roll_labels wrote
 * it; intr as above (it gives tx, ty).  One thread per output pixel, as preprocess_kernel.
 *   A row whose (c, sn) is exactly (1, 0) runs preprocess_px.inc itself: bit-identical to apg_synth_crops / ap_preprocess_crops.
 *   A rolled row takes the un-rolled box's h, w, scale, dw, dh, the pads and, for output pixel (ox, oy), dx = ox - left, dy = oy -
 *     top exactly as preprocess_px.inc computes them.  Padding pixels (outside 0 <= dx < dw, 0 <= dy < dh) are written as
 *     preprocess_px writes them: (0 - mean) / std.  A content pixel takes the source position BEFORE the floor, fx_ =
 *     (float)((dx + 0.5) * (1.0 / ((double)dw / (double)w)) - 0.5) and fy_ likewise (fp64, each operation rounded once, then one
 *     rounding to fp32), and samples the canvas at
 *         q = (x0 + hw, y0 + hh) + A(-theta) (fx_ - hw, fy_ - hh).
 *     The sample is bilinear with the zero continuation: a tap outside the canvas contributes 0, so the image is continuous in q.
 *     Unless -1 < q_x < Wc and -1 < q_y < Hc no tap lies on the canvas and the value is 0.  Else i = floor(q), a = q - i, a tap is
 *     byte / 255 of channel (2 - ch when bgr), top = (t00 * (1 - a_x)) + (t01 * a_x), bot likewise, v = (top * (1 - a_y)) +
 *     (bot * a_y).  Then (v - mean) / std, mean 0.485, 0.456, 0.406, std 0.229, 0.224, 0.225.
 *   A row whose box breaks 0 <= y0 < y1 <= Hc, 0 <= x0 < x1 <= Wc is neither read through nor written, as in apg_synth_crops.
 *
 * apg_roll_draw writes rot (2, n, 2) and nothing else: one thread per (s, i).  Philox4x32-10, key = (seed's low word, seed's high
 * word), counter = (index[i], epoch, camera, 15): block 15, camera 0 / 1, which no other stream uses (apg_synth_batch block 0,
 * apg_augment_draw blocks 1 .. 14, the noise blocks >= 2^31).  u = (word >> 8) * 2^-24.  Word 0 is the gate, on when u < p; word 1
 * the angle, ((2 * u) - 1) * max_rad in fp32; cos and sin of that fp32 angle are taken in fp64 and rounded once.  Gate off gives
 * exactly (1, 0); so do p = 0 and max_rad = 0.  A draw depends on (seed, index, epoch, camera) alone.
 *
 * APG_EINVAL before any GPU call, the message naming the argument: n outside 1 .. 65535, a NULL or misaligned pointer (cam may be
 * NULL; a label may be NULL, its output is needed when it is not), cam_all outside 0 .. 1, p outside 0 .. 1, max_rad outside 0 .. pi,
 * a canvas side outside 1 .. 2^20, V outside 1 .. 2^24, J or P outside 1 .. 2^16, pstride other than 2 or 3, bgr outside 0 .. 1, an
 * output overlapping its input, im overlapping a canvas. */
#define APG_ROLL_THREADS 256
#define APG_ROLL_CENTRE_OUT 1
#define APG_ROLL_OFF_CANVAS 2
int apg_roll_draw(int n, uint64_t seed, int epoch, const int* index, const int* cam, int cam_all, float p, float max_rad, float* rot,
                  void* stream);
int apg_roll_labels(int n, int V, int J, int P, int pstride, int Hc0, int Wc0, int Hc1, int Wc1, const int* cam, int cam_all,
                    const float* rot, const float* intr, const float* bb, const int* crops, const float* verts, const float* joints,
                    const float* orient, const float* trans, const float* extr, const float* j2d, const float* j2d_crop,
                    float* rot_used, float* bb_out, int* status, float* verts_out, float* joints_out, float* orient_out,
                    float* trans_out, float* extr_out, float* j2d_out, float* j2d_crop_out, void* stream);
int apg_roll_crops(int n, int Hc0, int Wc0, int Hc1, int Wc1, int bgr, const unsigned char* frames0, const unsigned char* frames1,
                   const int* cam, int cam_all, const int* crops, const float* intr, const float* rot_used, float* im, void* stream);

#ifdef __cplusplus
}
#endif
#endif
