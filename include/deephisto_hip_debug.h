/* deephisto_hip_debug.h -- TEST HOOKS of libdeephisto_hip.so.  NOT part of the drop-in boundary and NOT versioned.
 *
 * include/deephisto_hip.h is the boundary SURVEY.md section 8(b) describes (ABI version dh_abi_version()); the entry points below
 * exist so that tests/ can run ONE kernel of the engines on caller-provided data and localise an error to it (per-kernel parity
 * against float64 autograd, tests/test_gpu_train_kernels.py; single conv layers, tests/test_gpu_resnet.py; the cycle-stamped
 * diagnostic variants, tools/conv_stamps.py).  They are exported by the same shared object and bound by deephisto_amd/_lib.py,
 * but their signatures follow the kernels' internals and may change in any build without a change of dh_abi_version();
 * the product path (the deephisto_amd package, bench.py's timed region) never calls them.
 */
#ifndef DEEPHISTO_HIP_DEBUG_H
#define DEEPHISTO_HIP_DEBUG_H

#include "deephisto_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Taps of the training engines: float32 copy of a tensor the last forward / backward left in device memory, channels last.
 *   what = 0  Z  of conv `conv_name`: its raw output [B][Ho][Wo][cout]
 *   what = 1  Y: the BN (+ identity) (+ ReLU) output (bf16 stem: rebuilt from Z, the one tap that writes; float32 stem: refused, not kept)
 *   what = 2  dZ: the gradient with respect to Z exactly as the conv's weight-gradient kernel read it, [B][Ho][Wo][cout].  Only engines
 *             created with the side stream (DH_T2_SIDE / DH_T1_SIDE, the default) keep a dZ per conv, and only between a backward and
 *             the next forward is it this step's: refused otherwise.
 *   what = 3  with conv_name "conv1": X1, the pooled block input [B][H2][H2][64]; refused for any other name.
 * Refused with DH_EINVAL (dh_last_error names the argument): an unknown conv_name, what outside 0..3, n_elem other than the tensor's size.
 * Stream-ordered, no synchronisation.  dh_train2_debug_act: the bf16 engine; dh_resnet18_train_debug_act: the float32 engine. */
int dh_train2_debug_act(dh_train2* net, const char* conv_name, int32_t what, float* out_dev, int64_t n_elem, void* stream);
int dh_resnet18_train_debug_act(dh_resnet18* net, const char* conv_name, int32_t what, float* out_dev, int64_t n_elem, void* stream);

/* dh_train2_debug_backward_tap: dh_train2_backward (same dlogits, no fused Adam, the side stream as configured; the same host code with the
 * same launches in the same order) that also copies out, stream-ordered, what the backward of ONE batch norm -- named by its conv, as above --
 * read and wrote, each copy enqueued after the tensor's writer and before the buffer's next writer:
 *   grad_in_dev  float32[n_elem]: the tensor that BN's backward read as dy, [B][Ho][Wo][cout]: dOut for a block's top conv, dY for the others,
 *                the identity gradient for a downsample BN; for "conv1" the POOLED gradient [B][Hp][Wp][64] (the stem never materialises dY)
 *   g_out_dev    float32[n_elem]: the masked gradient that BN wrote.  Only the top BN of a block that is not pre-masked writes one: NULL for
 *                every other BN, a non-NULL pointer there is refused; NULL is accepted everywhere
 *   mean_dev, invstd_dev  float32[cout]: the saved forward statistics the backward kernels read
 *   route_host   int32[8], plain host values, complete when the call returns:
 *                [0] ReLU mode: 0 none / dy arrives masked, 1 pattern of the stored Y, 2 recomputed from Z
 *                [1] 1: the BN's block is pre-masked (its successor's dgrad GEMM masked the block's incoming gradient)
 *                [2] 1: the dgrad of the block's first conv masked its output with the predecessor's ReLU pattern (in_mask)
 *                [3] have_rows as passed in: rows of BN-backward sums a 1x1 dgrad GEMM's epilogue left for this BN (0: own reduction)
 *                [4] the reduction that ran: 0 none (epilogue sums), 1 channel-sliced, 2 bn2_bwd_reduce_kernel, 3 the stem's pool reduction
 *                [5] 1 fold (bn2_fold_bwd_apply_kernel), 2 finalize launch + apply pass
 *                [6] 0 a block without a downsample branch (or the stem), 1 a conv of a block with one, 2 the downsample BN itself
 *                [7] partial rows the finalize / fold read
 * Refused with DH_EINVAL (dh_last_error names the argument): a null argument other than g_out_dev / stream, an unknown conv_name, n_elem
 * other than grad_in's size, g_out_dev where no masked gradient is written, and no training forward since the last backward: a tapped
 * backward follows a forward of its own (after a backward the engine's state is that of a finished step; tests re-run the forward). */
int dh_train2_debug_backward_tap(dh_train2* net, const float* dlogits_dev, const char* conv_name, float* grad_in_dev, int64_t n_elem,
                                 float* g_out_dev, float* mean_dev, float* invstd_dev, int32_t* route_host, void* stream);

/* test hooks of the engine's GEMM-shaped kernels on caller data (bf16 bits as uint16; synchronise; `repeat` launches for timing):
 * gemm1x1: out[M][N] = A[rows][K] . W[N][K]^T (+ res), stride 2 = row gather (b, 2 oy, 2 ox) from [B][Hi][Wi][K];
 * wgrad:   float32 dW[cout][cin][ks][ks] from x [B][Hi][Wi][cin] and dz [B][Ho][Wo][cout] (ks 1 or 3). */
/* both bf16 operators of float32 w[cout][cin][3][3]: the engine's re-pack kernel (..._tile) and the element-wise packer (..._elem) */
int dh_debug_pack_bf16(const float* w_dev, int32_t cout, int32_t cin, uint16_t* wf_tile, uint16_t* wd_tile, uint16_t* wf_elem,
                       uint16_t* wd_elem, void* stream);
int dh_debug_gemm1x1_bf16(const uint16_t* a_dev, const uint16_t* w_dev, const uint16_t* res_dev, uint16_t* out_dev, int64_t M,
                          int32_t N, int32_t K, int32_t stride, int32_t Ho, int32_t Wo, int32_t Hi, int32_t Wi, int32_t repeat,
                          void* stream);
/* dh_debug_gemm1x1_fused_bf16: the 1x1 GEMM with its fused epilogues -- + res, ReLU mask of another tensor (output zeroed where
 * mask_dev <= 0), batch statistics of the bf16-rounded output (mean / invstd as the BN finalize writes them; both or neither). */
int dh_debug_gemm1x1_fused_bf16(const uint16_t* a_dev, const uint16_t* w_dev, const uint16_t* res_dev, const uint16_t* mask_dev,
                                uint16_t* out_dev, float* mean_dev, float* invstd_dev, int64_t M, int32_t N, int32_t K, int32_t stride,
                                int32_t Ho, int32_t Wo, int32_t Hi, int32_t Wi, int32_t repeat, void* stream);
/* dh_debug_gemm1x1_bwdsums_bf16: the dgrad GEMM whose output is the dY of a batch norm, with that BN's backward sums fused into the
 * epilogue: sums_dev[0..N) = sum g, sums_dev[N..2N) = sum g xhat (relu_mode 0: g = out as stored; 2: the BN's ReLU recomputed from z). */
int dh_debug_gemm1x1_bwdsums_bf16(const uint16_t* a_dev, const uint16_t* w_dev, const uint16_t* res_dev, const uint16_t* mask_dev,
                                  uint16_t* out_dev, const uint16_t* z_dev, const float* mean_dev, const float* invstd_dev,
                                  const float* scale_dev, const float* shift_dev, int32_t relu_mode, float* sums_dev, int64_t M, int32_t N,
                                  int32_t K, void* stream);
/* dh_debug_bn2_bf16: the bf16 engine's batch-norm kernels on caller data ([rows][C] channels-last, bf16 bits): forward with batch
 * statistics (y, saved mean / invstd), and, when dy_dev is given, backward (dz, dgamma, dbeta; relu_mode 0 none, 1 mask from y,
 * 2 mask recomputed from z; g_out_dev: the masked gradient, may be null). */
int dh_debug_bn2_bf16(const uint16_t* z_dev, const uint16_t* res_dev, const float* gamma_dev, const float* beta_dev, int32_t relu,
                      uint16_t* y_dev, float* mean_dev, float* invstd_dev, const uint16_t* dy_dev, int32_t relu_mode, uint16_t* dz_dev,
                      uint16_t* g_out_dev, float* dgamma_dev, float* dbeta_dev, int64_t rows, int32_t C, void* stream);
/* dh_debug_bn2_paths_bf16: dh_debug_bn2_bf16 with the engine's other routes through the same launch code selectable.  fold: 1 = small
 * maps (rows <= DH_T2_FOLD_ROWS) finalize inside the apply passes, 0 = partial sums -> finalize launch -> elementwise pass everywhere.
 * bits_dev (may be null): the ReLU pattern of y, [rows][C / 8] bytes, bit e set where value e of the 8 is non-zero.  z2_dev, gamma2_dev,
 * beta2_dev, mean2_dev, invstd2_dev (all or none): the join of a downsample block, y = relu(bn(z) + bf16(bn2(z2))), the branch BN's
 * statistics returned in mean2 / invstd2 (needs relu = 1 and no res_dev).  Every refusal names its argument (dh_last_error). */
int dh_debug_bn2_paths_bf16(const uint16_t* z_dev, const uint16_t* res_dev, const float* gamma_dev, const float* beta_dev, int32_t relu,
                            int32_t fold, uint16_t* y_dev, uint8_t* bits_dev, float* mean_dev, float* invstd_dev, const uint16_t* z2_dev,
                            const float* gamma2_dev, const float* beta2_dev, float* mean2_dev, float* invstd2_dev, const uint16_t* dy_dev,
                            int32_t relu_mode, uint16_t* dz_dev, uint16_t* g_out_dev, float* dgamma_dev, float* dbeta_dev, int64_t rows,
                            int32_t C, void* stream);
/* the stem's fused tail (bf16 engine): pooled = maxpool3x3/2(relu(bn(z))) straight from z with batch statistics (+ positions, mean, invstd);
 * with dpool_dev: dz, dgamma, dbeta with the maxpool's gradient gathered inside the BN backward passes. */
int dh_debug_bn2_pool_bf16(const uint16_t* z_dev, const float* gamma_dev, const float* beta_dev, uint16_t* pooled_dev, uint8_t* idx_dev,
                           float* mean_dev, float* invstd_dev, const uint16_t* dpool_dev, uint16_t* dz_dev, float* dgamma_dev,
                           float* dbeta_dev, int32_t B, int32_t Hi, int32_t Wi, int32_t C, void* stream);
/* The remaining HBM-bound kernels of the bf16 engine on caller data: max-pool 3x3/2 forward (+ backward when dy_dev is given),
 * the strided add of the downsample branch's gradient, and the average-pool + fc backward. */
int dh_debug_maxpool2_bf16(const uint16_t* x_dev, uint16_t* y_dev, const uint16_t* dy_dev, uint16_t* dx_dev, int32_t B, int32_t Hi,
                           int32_t Wi, int32_t C, void* stream);
/* ... the same max-pool pair, with the recorded first-maximum positions returned: idx_dev [B][Ho][Wo][C] bytes, dyy * 3 + dxx. */
int dh_debug_maxpool2_idx_bf16(const uint16_t* x_dev, uint16_t* y_dev, uint8_t* idx_dev, const uint16_t* dy_dev, uint16_t* dx_dev, int32_t B,
                               int32_t Hi, int32_t Wi, int32_t C, void* stream);
int dh_debug_upsample2_add_bf16(const uint16_t* t_dev, uint16_t* dx_dev, int32_t B, int32_t Ho, int32_t Wo, int32_t Hi, int32_t Wi,
                                int32_t C, void* stream);
int dh_debug_avgpool_fc_dgrad2(const float* dlogits_dev, const float* w_dev, uint16_t* dx_dev, int32_t B, int32_t HW, int32_t C,
                               int32_t n_cls, void* stream);
int dh_debug_stem_wgrad_bf16(const uint16_t* dz_dev, const float* x_nchw_dev, float* dw_dev, int32_t B, int32_t P, void* stream);
/* dh_debug_head: the classifier head of both training engines on caller data, in the order a step launches it: global average pool
 * (x_bf16 = 0: the float32 engine's kernel on float32 x; 1: the bf16 engine's on bf16 bits), fc forward, fc weight / bias gradient from
 * the caller's dlogits and the pooled features just made, and the matching average-pool + fc data gradient (dx float32 / bf16 bits).
 * x, dx [B][HW][C]; w [n_cls][C]; bias [n_cls]; dlogits, logits [B][n_cls]; pooled [B][C]; dw [n_cls][C]; db [n_cls].  Every output is
 * written in full.  Refused (DH_EINVAL, dh_last_error names the argument): a null pointer, x_bf16 outside {0, 1}, B, HW or n_cls < 1,
 * C not a positive multiple of 8.  Synchronises. */
int dh_debug_head(const void* x_dev, int32_t x_bf16, const float* w_dev, const float* bias_dev, const float* dlogits_dev,
                  float* pooled_dev, float* logits_dev, float* dw_dev, float* db_dev, void* dx_dev, int32_t B, int32_t HW, int32_t C,
                  int32_t n_cls, void* stream);
int dh_debug_wgrad_bf16(const uint16_t* dz_dev, const uint16_t* x_dev, float* dw_dev, int32_t B, int32_t Hi, int32_t Wi,
                        int32_t cin, int32_t cout, int32_t ks, int32_t stride, int32_t repeat, void* stream);
/* dh_debug_conv_bf16: ONE convolution of the bf16 training engine on caller data (bf16 bits, NHWC), forward or data gradient, exactly as a
 * step launches it: both operands are packed from float32 w[cout][cin][ks][ks] by the step's packer, and the step's own dispatch picks the
 * tile and the variant (nothing of that choice is restated in the hook).  Hi x Wi is always the convolution's INPUT size.
 *   dgrad = 0: in = x [B][Hi][Wi][cin],   out = Z [B][Ho][Wo][cout], raw (no epilogue); res must be null
 *   dgrad = 1: in = dZ [B][Ho][Wo][cout], out = dX [B][Hi][Wi][cin] (+ res, the gradient joining from another branch; may be null).
 *              1x1 / stride 2 follows the engine's accumulate contract: out starts from res (or zero), the low-resolution product is
 *              stored as bf16 and then added into it (two stored roundings).
 * Refused (dh_last_error names the argument): ks outside {1, 3}, stride outside {1, 2}, cin / cout not multiples of 64, and an odd Hi or
 * Wi at stride 2 -- the engine requires P % 32 == 0, so every map in front of a stride-2 convolution is even and odd ones are
 * unreachable in bf16 (the float32 engine's odd maps: dh_debug_dgrad_f32).  Synchronises. */
int dh_debug_conv_bf16(const uint16_t* in_dev, const float* w_dev, const uint16_t* res_dev, uint16_t* out_dev, int32_t B, int32_t Hi,
                       int32_t Wi, int32_t cin, int32_t cout, int32_t ks, int32_t stride, int32_t dgrad, void* stream);

/* ---- debug / test hooks (not part of the drop-in boundary) ---------------------
 * dh_debug_conv_bn_act: one conv (ks in {1,3}, pad ks/2) + per-channel scale/shift
 * (+ residual) (+ ReLU) on NHWC data of `dtype`; weights are float32
 * [cout][cin][ks][ks] on the host.  Synchronises the stream.
 * dh_debug_stem_out: float32 NHWC copy of the stem activation (conv1+bn1+relu) left
 * in the workspace by the last forward of n tiles of size P. */
int dh_debug_conv_bn_act(const void* in_dev, const float* w_host, const float* scale_host,
                         const float* shift_host, const void* res_dev, void* out_dev, int32_t B,
                         int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t ks, int32_t stride,
                         int32_t relu, int32_t dtype, void* stream);
int dh_debug_stem_out(dh_resnet18* net, int64_t n, int32_t patch, float* out_dev, void* stream);
/* dh_debug_stem_pool_bf16: the fused bf16 stem (conv1 + bn1 + relu + maxpool, models/patch_cls_simple/model.py:6 = the first four
 * modules of torchvision's resnet18) of n tiles read from the uint8 slide, as float32 NHWC [n][H2][W2][64]; synchronises. */
int dh_debug_stem_pool_bf16(dh_resnet18* net, const uint8_t* slide_dev, int64_t slide_h, int64_t slide_w, const int32_t* yx_dev,
                            int64_t n, int32_t patch, float* out_dev, void* stream);
/* Backward building blocks of the float32 training engine, one at a time, exactly as dh_resnet18_backward launches them
 * (all tensors float32 on the device, activations NHWC; each call allocates its own scratch and synchronises):
 *   wgrad       dW[cout][cin][ks][ks] from x [B][Hi][Wi][cin] and dz [B][Ho][Wo][cout]; mode 1 forces the per-tap kernel
 *   stem_wgrad  dW[64][3][7][7] from the NCHW image and dz [B][P/2][P/2][64]
 *   dgrad       dX from dz and the weights [cout][cin][ks][ks] (+ res): stride 2 = the four parity classes of dX over dz
 *               itself (3x3) / low-resolution product scattered back (1x1)
 *   bn          training-mode BN forward (+ res, ReLU) and, when dy is given, backward (dz, masked gradient g, dgamma, dbeta);
 *               relu: 0 none, 1 ReLU with the backward pattern read from y, 2 ReLU with the pattern recomputed from z (the
 *               engine's path for a BN that feeds a ReLU directly; res_dev and g_dev must be NULL, refused otherwise);
 *               stats_out = [mean | invstd | running_mean | running_var] after one update from (0, 1)
 *   maxpool     3x3/2 forward and (dy given) backward through the recorded first-maximum positions */
int dh_debug_wgrad_f32(const float* dz_dev, const float* x_dev, float* dw_dev, int32_t B, int32_t Hi, int32_t Wi,
                       int32_t cin, int32_t cout, int32_t ks, int32_t stride, int32_t mode, void* stream);
int dh_debug_stem_wgrad_f32(const float* dz_dev, const float* x_nchw_dev, float* dw_dev, int32_t B, int32_t P, void* stream);
int dh_debug_dgrad_f32(const float* dz_dev, const float* w_dev, const float* res_dev, float* dx_dev, int32_t B, int32_t Hi,
                       int32_t Wi, int32_t cin, int32_t cout, int32_t ks, int32_t stride, void* stream);
/* both packed operators of w[cout][cin][3][3]: the training step's sub-tile kernel (..._tile) and the element-wise kernel (..._elem) */
int dh_debug_pack_f32(const float* w_dev, int32_t cout, int32_t cin, float* wf_tile, float* wd_tile, float* wf_elem, float* wd_elem,
                      void* stream);
int dh_debug_bn_f32(const float* z_dev, const float* gamma_dev, const float* beta_dev, const float* res_dev, int32_t relu,
                    float* y_dev, const float* dy_dev, float* dz_dev, float* g_dev, float* dgamma_dev, float* dbeta_dev,
                    float* stats_out_dev, int64_t rows, int32_t C, void* stream);
int dh_debug_maxpool_f32(const float* x_dev, float* y_dev, const float* dy_dev, float* dx_dev, int32_t B, int32_t Hi, int32_t Wi,
                         int32_t C, void* stream);
/* the stem's fused tail (float32 engine): pooled = maxpool3x3/2(relu(bn(z))) straight from z with batch statistics (+ positions); with
 * dpool_dev: dz, dgamma, dbeta with the maxpool's gradient gathered inside the BN backward passes */
int dh_debug_bn_pool_f32(const float* z_dev, const float* gamma_dev, const float* beta_dev, float* pooled_dev, uint8_t* idx_dev,
                         const float* dpool_dev, float* dz_dev, float* dgamma_dev, float* dbeta_dev, int32_t B, int32_t Hi, int32_t Wi,
                         int32_t C, void* stream);
/* dh_debug_stem_strip_width: pooled columns per column strip of the fused bf16 stem for every later launch of the process: 15
 * (independent strips), 16 (aligned strips joined by stem_seam_kernel), or 0 = chosen by geometry, the default: 16 where that
 * needs fewer strips.  The stem's output does not depend on it, bit for bit (tests/test_gpu_stem_strips.py). */
int dh_debug_stem_strip_width(int32_t pooled_columns);
/* dh_debug_stamps: switch the 3x3-conv kernel to its cycle-stamped diagnostic variant and/or read
 * (and clear) its 8x8 table of summed phase cycles; out64_host may be NULL. */
int dh_debug_stamps(int32_t enable, unsigned long long* out64_host);
/* dh_debug_last_conv3: what the process's last 3x3 convolution launch ran -- *variant: the stride-1 tile variant (0 / 1 / 2 = 512 / 256 / 128
 * pixels per workgroup; -1: a stride-2 launch or a parity class of a data gradient), *mfma_m: 16 = 16x16x32 MFMAs, 32 = 32x32x16. */
int dh_debug_last_conv3(int32_t* variant, int32_t* mfma_m);
/* dh_debug_env_knobs: the table of every environment variable the library reads (csrc/env_knobs.h), one "NAME default lo hi read"
 * line per knob, NUL-terminated, into buf_host[cap]; INTEGRATION.md lists the same table (tests/test_abi.py compares them). */
int dh_debug_env_knobs(char* buf_host, int64_t cap);

/* Per-layer taps of the inference engines.  dh_debug_*_forward_tap runs the launches of dh_*_forward_tiles for all n tiles and, right after
 * the launch that stores conv `conv_name`'s output (a state_dict conv name; "maxpool" = the pooled stem output, which the fused bf16 stems
 * also store under "conv1"; the float32 ResNet-18 stores "conv1" = relu(bn1(conv1)) before its pool), copies that stored activation of the
 * images sel_dev[0..k) as float32 NCHW [k][C][H][W] into out_dev (out_elems = k*C*H*W), stream-ordered before any later launch overwrites
 * it; logits_dev receives the logits of the same run.  Refused (dh_last_error) for an unknown name, k outside [1, n], or a sel outside
 * [0, n) (read back: one synchronisation).  dh_debug_*_operands: conv `conv_name`'s operands as the engine holds them after finalize,
 * read back from the device into host buffers: the weight unpacked to float32 [cout][cin][ks][ks] (bf16 engines: bf16-rounded;
 * ResNet-50: BN folded, then rounded), scale and shift [cout] (ResNet-50: 1 and the folded bias); synchronous. */
int dh_debug_resnet18_forward_tap(dh_resnet18* net, const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx_dev, int64_t n, int32_t P,
                                  const char* conv_name, const int32_t* sel_dev, int32_t k, float* out_dev, int64_t out_elems,
                                  float* logits_dev, void* stream);
int dh_debug_resnet50_forward_tap(dh_resnet50* net, const uint8_t* slide, int64_t h, int64_t w, const int32_t* yx_dev, int64_t n, int32_t P,
                                  const char* conv_name, const int32_t* sel_dev, int32_t k, float* out_dev, int64_t out_elems,
                                  float* logits_dev, void* stream);
int dh_debug_resnet18_operands(dh_resnet18* net, const char* conv_name, float* w_host, int64_t w_elems, float* scale_host,
                               float* shift_host, int64_t c_elems);
int dh_debug_resnet50_operands(dh_resnet50* net, const char* conv_name, float* w_host, int64_t w_elems, float* scale_host,
                               float* shift_host, int64_t c_elems);

/* dh_debug_coverage_set_map: replace a coverage handle's map by int32 host counts [dh][dw] (>= 0) and recount its per-chunk
 * eligible counts, filled and eligible (tests of the rank -> cell and compaction kernels on crafted maps); synchronises `stream`. */
int dh_debug_coverage_set_map(dh_coverage* cov, const int32_t* map_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEEPHISTO_HIP_DEBUG_H */
