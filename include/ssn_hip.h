/* ssn_hip.h -- C ABI of libssn_hip.so: the MI355X (gfx950) kernels behind the SSN hot path.
 *
 * The reference (yjxiong/action-detection) has no FFI layer: its hot path is Python that calls
 * torch ops, which in turn call cuDNN / cuBLAS.  Each entry point below replaces one of those
 * implicit native calls; the reference call site it stands in for is cited per function
 * (paths relative to /root/reference).  The Python mirror of the reference's nn.Module API
 * (action-detection_amd/ssn_models.py, ops/ssn_ops.py) binds these with ctypes; INTEGRATION.md
 * shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *  - every buffer is device memory owned by the caller (PyTorch); the library allocates nothing
 *    persistent and never synchronises the stream;
 *  - tensors are fp32, NCHW, W-contiguous; "img_stride" arguments are the float distance between
 *    consecutive images, so a channel slice of a wider (concat) tensor is addressed by offsetting
 *    the base pointer to the slice's first channel and passing the wide tensor's C*H*W;
 *  - index / label tensors are int64 as in the reference;
 *  - return value: 0 on success, negative SSN_ERR_* otherwise (message: ssn_last_error());
 *    nothing throws across the ABI;
 *  - all launches go to `stream` (the caller's current HIP stream); re-entrant per stream.
 */
#ifndef SSN_HIP_H
#define SSN_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

#define SSN_ERR_ARG (-1)
#define SSN_ERR_LAUNCH (-2)
#define SSN_ERR_WORKSPACE (-3)

const char* ssn_last_error(void);
int ssn_abi_version(void);   /* 9 */

/* ------------------------------------------------------------------ backbone: conv + BN + ReLU
 * Weight re-layout for the implicit-GEMM kernels (what cuDNN does internally with its filter
 * descriptors): w is the torch-layout [Cout][Cin][k][k] weight; `packed` receives
 * ssn_conv_packed_floats() floats.  transposed=0 -> operand of the forward conv, 1 -> of dgrad,
 * 2 -> of the parity-ordered stride-2 dgrad (see ssn_conv_dgrad_layout). */
long ssn_conv_packed_floats(int Cout, int Cin, int ksize, int transposed);
int ssn_conv_pack_weights(const float* w, float* packed, int Cout, int Cin, int ksize, int transposed,
                          hipStream_t stream);

/* The same for `count` layers in ceil(count/40) launches; every argument is a HOST array with one entry per
 * layer.  w1/split describe the optional second source of a fused pair (output channels >= split come from w1);
 * pass w1 = NULL and split = cout otherwise. */
int ssn_conv_pack_weights_multi(int count, const float* const* w0, const float* const* w1, float* const* out,
                                const int* cout, const int* cin, const int* ksize, const int* mode, const int* split,
                                hipStream_t stream);

/* Replaces cuDNN conv fwd + cudnnBatchNorm(eval) + ReLU of every "conv / bn / relu" triple of
 * model_zoo.BNInception, reached from ssn_models.py:266 (train) and :298 (test).
 * y[n][co][ho][wo] = relu?( scale[co] * sum_{ci,r,s} w[co][ci][r][s] * x[n][ci][ho*S-pad+r][wo*S-pad+s]
 *                           + shift[co] )        scale/shift may be NULL (plain convolution).
 * ksize in {1,3,7}, stride in {1,2}.  tile_cfg < 0 selects the tile heuristically.
 * w_packed = ssn_conv_pack_weights(w, transposed=0). */
int ssn_conv_bn_relu_fwd(const float* x, const float* w_packed, const float* scale, const float* shift, float* y,
                         int N, int Cin, int H, int W, long x_img_stride, int Cout, int Ho, int Wo,
                         long y_img_stride, int ksize, int stride, int pad, int relu, int tile_cfg,
                         float* y_amax, hipStream_t stream);   /* y_amax: see "amax slots" below; NULL = not tracked */

/* Frozen-BN folding (ssn_models.py:156-174 puts every BatchNorm2d in eval mode):
 * scale = gamma / sqrt(var + eps), shift = (conv_bias - mean) * scale + beta. */
int ssn_bn_fold(const float* conv_bias, const float* gamma, const float* beta, const float* mean,
                const float* var, float eps, float* scale, float* shift, int C, hipStream_t stream);

/* ssn_bn_fold for `count` layers in ceil(count/48) launches; every argument is a HOST array with one entry
 * per layer (device pointers, eps, channel count). */
int ssn_bn_fold_multi(int count, const float* const* conv_bias, const float* const* gamma, const float* const* beta,
                      const float* const* mean, const float* const* var, const float* eps, float* const* scale,
                      float* const* shift, const int* channels, hipStream_t stream);

/* Backward of ReLU + frozen BN, in place on dy:  dy <- dy * (y > 0) * scale[c]
 * (autograd of the same triples, entered from ssn_train.py:236 loss.backward()). */
int ssn_relu_bn_bwd(float* dy, const float* y, const float* scale, int N, int C, int HW, long dy_img_stride,
                    long y_img_stride, float* dy_amax, hipStream_t stream);

/* cuDNN dgrad replacement.  wt_packed = ssn_conv_pack_weights(w, transposed=1).
 * dx[n][ci][hi][wi] (+)= sum_{co,r,s} w[co][ci][r][s] * dy[n][co][(hi+pad-r)/S][(wi+pad-s)/S].
 * mask_y / mask_scale (optional, both or neither): when this call is the last writer of dx, the
 * backward of the ReLU + frozen BN that produced the tensor dx belongs to is fused into the store:
 * dx <- dx * (mask_y > 0) * mask_scale[ci]   (mask_scale[ci] NaN: not a ReLU output, dx unchanged;
 * finite scales of either sign are applied as they are).
 * wt_layout = ssn_conv_dgrad_layout(...): 2 selects the parity-ordered stride-2 path (3x3/s2/p1, even input),
 * whose weights must have been packed with transposed = 2; otherwise 1. */
int ssn_conv_dgrad_layout(int ksize, int stride, int pad, int H, int W);
int ssn_conv_dgrad(const float* dy, const float* wt_packed, float* dx, int N, int Cout, int Ho, int Wo,
                   long dy_img_stride, int Cin, int H, int W, long dx_img_stride, int ksize, int stride,
                   int pad, int accumulate, const float* mask_y, long mask_img_stride, const float* mask_scale,
                   int wt_layout, int tile_cfg, float* dx_amax, hipStream_t stream);

/* ---- amax slots (operand scaling of the split kernels below).  A slot is ONE float in device memory holding an
 * upper bound of max |t| of a tensor t; the caller zeroes it before the first kernel writes t, every kernel of this
 * library that stores into t and is handed the slot (the *_amax output arguments; NULL = t is not tracked) raises
 * it to the largest magnitude it stores (unsigned atomic max on the bit pattern), and the split kernels that READ t
 * as a matrix operand derive its power-of-two f16 scale from the slot (the const *_amax arguments, required).
 * ssn_tensor_amax does the same for a tensor no library kernel produced (the frames handed in by the caller). */
int ssn_tensor_amax(const float* x, long n, float* slot, hipStream_t stream);

/* ---- "x6" variants: the same convolutions computed on the f16 matrix cores with fp32-class accuracy ("x6" is the
 * family's historical name: its first version multiplied six bf16 partial products).
 * Every fp32 operand, scaled by a per-tensor power of two, is split into two f16 terms (11+11 significand bits,
 * round to nearest) and the product is accumulated in fp32 from the three partial products a_lo*b_hi + a_hi*b_hi +
 * a_hi*b_lo (csrc/conv_x6.hip); the dropped term is <= 2^-22 |ab|, and the measured error against float64 stays
 * within 2x of an fp32 FMA chain (the 1e-4 budget of the path is untouched) at 3/16 of the f32-MFMA matrix time.
 * ksize in {1,3}; forward stride in {1,2}; dgrad stride 1.
 * Weights: ssn_conv_x6_pack_weights_multi (mode 0 forward / 1 dgrad operand; same w1/split convention as
 * ssn_conv_pack_weights_multi; measures max |w|, scales, splits and packs), ssn_conv_x6_packed_floats() floats per layer.
 * x_amax / dy_amax (required): amax slot of the tensor the gathered operand lives in; y_amax / dx_amax: slot of the
 * output tensor or NULL.
 * x_guard_bytes / dy_guard_bytes: how many bytes directly in FRONT of the gathered tensor the caller guarantees to
 * be readable device memory (e.g. the channels below a channel slice, or an allocation pad).  With >= 256 the
 * stride-1 kernels fetch activations 16 bytes per lane (4 consecutive pixels; border positions are zeroed later),
 * which reaches a few bytes before the first element; with 0 they use 4-byte loads and never leave the tensor.  Same call sites as
 * ssn_conv_bn_relu_fwd / ssn_conv_dgrad (ssn_models.py:266,298; loss.backward at ssn_train.py:223). */
long ssn_conv_x6_packed_floats(int Cout, int Cin, int ksize, int transposed);
void ssn_conv_x6_debug_trace(unsigned long long* per_block_8_words); /* tooling only; NULL = off */
void ssn_conv_x6_debug_flags(int flags);   /* tooling only (tools/ablate_x6.py); 0 = normal operation */
/* The fused launch on an Inception block input (1x1 branch + reduce pair + pool projection = ONE convolution):
 *  - w0..w3, split..split3: up to four weight sources per entry -- output channels [0, split) from w0, [split, split2)
 *    from w1, [split2, split3) from w2, the rest from w3; all splits = cout for a single source;
 *  - raw_from (fwd, > 0): output channels >= raw_from take neither the affine nor the ReLU (the bias-free projection);
 *  - row_split / row_gap (fwd; multiples of 32, 0 = none): output channels >= row_split are stored row_gap channels further
 *    up y's tensor (the 1x1 branch goes to the head of the block output, the rest behind the block's own channels);
 *  - k_split / k_gap (dgrad; multiples of 16): the same displacement on the channel axis of dy;
 *  - g_row_split / g_row_gap (wgrad): ... and on the rows of g;
 *  - y_amax2 / dy_amax2 / g_amax2 (NULL = none): such a tensor has ONE AMAX SLOT PER REGION (the block's own channels; the rows
 *    behind them), so that every slot is complete before anything reads it although the regions are written and read by
 *    concurrent launches; the launch that spans both raises both (fwd) resp. uses the larger of both (dgrad, wgrad). */
int ssn_conv_x6_pack_weights_multi(int count, const float* const* w0, const float* const* w1, const float* const* w2,
                                   const float* const* w3, float* const* out, const int* cout, const int* cin,
                                   const int* ksize, const int* mode, const int* split, const int* split2,
                                   const int* split3, hipStream_t stream);
/* Batched packing: every ssn_conv_x6_pack_* call between _begin and _end only RECORDS its entries; _end issues all of them in three
 * launches (clear the amax tails, max |w| per entry, pack) through a device-resident plan.  plan: >= ssn_conv_x6_pack_batch_entries()
 * * ssn_conv_x6_pack_entry_bytes() bytes of device memory the caller keeps from step to step; it is rewritten (ceil(entries / 40)
 * small launches) only when the recorded entries differ from the ones last written there, or with force_write (a buffer the caller
 * has just allocated).  _abort drops an open batch.  One batch at a time per process (one process per GPU). */
int ssn_conv_x6_pack_batch_begin(void);
int ssn_conv_x6_pack_batch_entries(void);
long ssn_conv_x6_pack_entry_bytes(void);
void ssn_conv_x6_pack_batch_abort(void);
int ssn_conv_x6_pack_batch_end(void* plan, long plan_bytes, int force_write, hipStream_t stream);
/* _end in two parts: the first n_first recorded entries (the stem's) on `stream`, the others on `side_stream`, forked behind the
 * plan writes of `stream`; a join event is recorded behind them, and ssn_conv_x6_pack_batch_join makes a stream wait for it (no
 * pending join: a no-op).  Events: once per device, no timing, never created inside a capture.  n_first == entries or a null
 * side_stream: exactly _end.  The packed bytes do not depend on where an entry runs. */
int ssn_conv_x6_pack_batch_end_lanes(void* plan, long plan_bytes, int force_write, int n_first, hipStream_t stream,
                                     hipStream_t side_stream);
int ssn_conv_x6_pack_batch_join(hipStream_t stream);
int ssn_conv_x6_fwd(const float* x, const float* w_packed, const float* scale, const float* shift, float* y, int N,
                    int Cin, int H, int W, long x_img_stride, int Cout, int Ho, int Wo, long y_img_stride,
                    int ksize, int stride, int pad, int relu, int x_guard_bytes, int tile_cfg, const float* x_amax,
                    float* y_amax, int raw_from, int row_split, int row_gap, float* y_amax2, hipStream_t stream);
int ssn_conv_x6_dgrad(const float* dy, const float* wt_packed, float* dx, int N, int Cout, int Ho, int Wo,
                      long dy_img_stride, int Cin, int H, int W, long dx_img_stride, int ksize, int pad,
                      int accumulate, const float* mask_y, long mask_img_stride, const float* mask_scale,
                      int dy_guard_bytes, int tile_cfg, const float* dy_amax, float* dx_amax, int k_split, int k_gap,
                      const float* dy_amax2, hipStream_t stream);

/* Rectangular taps (csrc/conv_x6_rect.hip): the forward convolutions of the Inception-v3 backbone the reference's
 * tester runs on ActivityNet (ssn_models.py:133-139): kh x kw in {5x5, 1x7, 7x1, 1x3, 3x1}, stride 1, per-axis
 * padding; same kernel, arguments and accuracy class as ssn_conv_x6_fwd.  Their data gradient (training SSN on
 * Inception-v3, ssn_models.py:133-139 + ssn_train.py:236) is the forward correlation of dy with the transposed,
 * tap-reversed weight (ssn_conv_x6_pack_dgrad_rect): ssn_conv_x6_dgrad_rect, same-size layers (2 pad = taps - 1),
 * accumulate / mask_y / mask_scale as ssn_conv_x6_dgrad. */
long ssn_conv_x6_packed_floats_rect(int Cout, int Cin, int kh, int kw);
int ssn_conv_x6_pack_weights_rect(const float* w, float* out, int cout, int cin, int kh, int kw, hipStream_t stream);
int ssn_conv_x6_fwd_rect(const float* x, const float* w_packed, const float* scale, const float* shift, float* y,
                         int N, int Cin, int H, int W, long x_img_stride, int Cout, int Ho, int Wo,
                         long y_img_stride, int kh, int kw, int pad_h, int pad_w, int relu, int x_guard_bytes,
                         int tile_cfg, const float* x_amax, float* y_amax, hipStream_t stream);
/* `count` rectangular-tap weights in one call (host arrays, one entry per layer); mode 0: forward operand, 2: dgrad operand */
int ssn_conv_x6_pack_rect_multi(int count, const float* const* w, float* const* out, const int* cout, const int* cin,
                                const int* kh, const int* kw, const int* mode, hipStream_t stream);
long ssn_conv_x6_packed_floats_dgrad_rect(int Cout, int Cin, int kh, int kw);
int ssn_conv_x6_pack_dgrad_rect(const float* w, float* out, int cout, int cin, int kh, int kw, hipStream_t stream);
int ssn_conv_x6_dgrad_rect(const float* dy, const float* wt_packed, float* dx, int N, int Cout, int H, int W,
                           long dy_img_stride, int Cin, long dx_img_stride, int kh, int kw, int pad_h, int pad_w,
                           int accumulate, const float* mask_y, long mask_img_stride, const float* mask_scale,
                           int dy_guard_bytes, int tile_cfg, const float* dy_amax, float* dx_amax, hipStream_t stream);

/* Data gradient of the 3x3 / stride-2 / pad-1 layers (even input size) on the x6 kernel: four stride-1 launches, one
 * per parity class of the input pixel, each multiplying only the taps that reach that class (cuDNN dgrad behind
 * loss.backward(), ssn_train.py:236).  wt_packed: ssn_conv_x6_pack_dgrad_s2 (ssn_conv_x6_dgrad_s2_packed_floats
 * floats) of the torch-layout weight [Cout][Cin][3][3].  pad = 1 (BN-Inception; even input size) or 0 (the "valid"
 * stride-2 layers of Inception-v3, any input size >= 3).  Other arguments as ssn_conv_x6_dgrad. */
long ssn_conv_x6_dgrad_s2_packed_floats(int Cout, int Cin);
int ssn_conv_x6_pack_dgrad_s2(const float* w, float* out, int cout, int cin, hipStream_t stream);
int ssn_conv_x6_dgrad_s2(const float* dy, const float* wt_packed, float* dx, int N, int Cout, int Ho, int Wo,
                         long dy_img_stride, int Cin, int H, int W, long dx_img_stride, int accumulate,
                         const float* mask_y, long mask_img_stride, const float* mask_scale, int dy_guard_bytes,
                         int tile_cfg, const float* dy_amax, float* dx_amax, int pad, hipStream_t stream);

/* x6 weight gradient (csrc/conv_wgrad_x6.hip): stride-1 same-size 1x1 / 3x3 convolutions with H*W % 4 == 0, both
 * operands scaled and split to f16 on the fly (g_amax / x_amax: their tensors' amax slots, required), 16-byte loads
 * along the pixel axis.  Same result contract as ssn_conv_wgrad
 * (deterministic split-K).  x_guard_bytes >= 256 is REQUIRED (the shifted taps read up to W+1 floats before x). */
long ssn_conv_wgrad_x6_workspace_bytes(int N, int Cin, int Cout, int H, int W, int ksize, int tile_cfg);
int ssn_conv_wgrad_x6(const float* g, const float* x, float* dw, float* db, int N, int Cin, int H, int W,
                      long x_img_stride, int Cout, long g_img_stride, int ksize, int pad, int x_guard_bytes,
                      void* workspace, long ws_bytes, int tile_cfg, const float* g_amax, const float* x_amax,
                      int g_row_split, int g_row_gap, const float* g_amax2, hipStream_t stream);
/* ... of the stride-1 same-size layers with rectangular taps (kh x kw, 2 pad = taps - 1; dw [Cout][Cin][kh][kw]); x needs
 * (pad_h * W + pad_w) * 4 readable bytes in front of it, rounded up to a multiple of 256.  pad_h = pad_w = 0: the taps reach
 * 0 .. k-1 pixels BEHIND the pixel -- the weight gradient of an unpadded convolution whose output gradient was laid into
 * planes of the input's size (ssn_embed_planes). */
long ssn_conv_wgrad_x6_rect_workspace_bytes(int N, int Cin, int Cout, int H, int W, int kh, int kw, int tile_cfg);
int ssn_conv_wgrad_x6_rect(const float* g, const float* x, float* dw, float* db, int N, int Cin, int H, int W,
                           long x_img_stride, int Cout, long g_img_stride, int kh, int kw, int pad_h, int pad_w,
                           int x_guard_bytes, void* workspace, long ws_bytes, int tile_cfg, const float* g_amax,
                           const float* x_amax, hipStream_t stream);
/* second pass of both wgrad kernels: dw[m][kk] = sum_z part[z][m][kk], db[m] = sum_z part[z][m][K] */
int ssn_wgrad_reduce(const float* part, float* dw, float* db, int M, int K, int splits, hipStream_t stream);
/* the same with TAP-MAJOR slab columns (column t * (K / taps) + ci holds dW[m][ci][t]): the nine-tap planes kernel's slabs */
int ssn_wgrad_reduce_taps(const float* part, float* dw, float* db, int M, int K, int splits, int taps, hipStream_t stream);

/* cuDNN wgrad (+ bias grad) replacement.  dw[co][ci][r][s] = sum_p g * x,  db[co] = sum_p g  (db may be NULL).
 * workspace: ssn_conv_wgrad_workspace_bytes() bytes of scratch for the split-K partial slabs. */
long ssn_conv_wgrad_workspace_bytes(int N, int Cin, int Cout, int Ho, int Wo, int ksize, int tile_cfg);
int ssn_conv_wgrad(const float* g, const float* x, float* dw, float* db, int N, int Cin, int H, int W,
                   long x_img_stride, int Cout, int Ho, int Wo, long g_img_stride, int ksize, int stride, int pad,
                   void* workspace, long ws_bytes, int tile_cfg, hipStream_t stream);
int ssn_conv_pick_tile(int M, long P);
/* tooling only: ablation switches for the conv kernel (tools/ablate_conv.py); 0 = normal operation */
int ssn_conv_debug_flags(int flags);

/* ------------------------------------------------------------------ backbone: training-mode BatchNorm2d
 * bn_mode 'partial' (first BatchNorm2d) / 'full' (all) of ssn_models.py:95-105,156-174 (csrc/bn_train.hip): the
 * layers SSN.train() leaves in training mode normalise with batch statistics, update running_mean / running_var
 * (momentum, unbiased variance) and take the full batch-norm backward.  z is the convolution output WITHOUT the conv
 * bias (it cancels in z - mean(z); conv_bias only enters the running mean).  workspace:
 * ssn_bn_train_workspace_floats(N, C) floats.  Reductions are two-level, atomic-free, combined in double.
 *   stats : mean[c], invstd[c] = 1/sqrt(biased var + eps) over (N, HW); running stats updated in place (or NULL)
 *   apply : y = relu?(gamma * (z - mean) * invstd + beta)
 *   bwd   : g = dy * (y > 0 | 1), dbeta = sum g, dgamma = sum g * xhat, dz = gamma * invstd * (g - dbeta/n - xhat * dgamma/n) */
long ssn_bn_train_workspace_floats(int N, int C);
int ssn_bn_train_stats(const float* z, const float* conv_bias, float* mean, float* invstd, float* running_mean,
                       float* running_var, int N, int C, int HW, long z_img_stride, float eps, float momentum,
                       void* workspace, size_t ws_bytes, hipStream_t stream);
int ssn_bn_train_apply(const float* z, float* y, const float* mean, const float* invstd, const float* gamma,
                       const float* beta, int relu, int N, int C, int HW, long z_img_stride, long y_img_stride,
                       float* y_amax, hipStream_t stream);
int ssn_bn_train_bwd(const float* dy, const float* y, const float* z, const float* mean, const float* invstd,
                     const float* gamma, float* dgamma, float* dbeta, float* dz, int relu, int N, int C, int HW,
                     long dy_img_stride, long y_img_stride, long z_img_stride, long dz_img_stride, void* workspace,
                     size_t ws_bytes, float* dz_amax, hipStream_t stream);

/* ------------------------------------------------------------------ backbone: pooling
 * Max / average pools of BN-Inception (ceil_mode output sizes computed by the caller, avg with
 * count_include_pad=True) and the global average pool before `fc` (ssn_models.py:266 -> backbone).
 * argmax: uint8 [N][C][Ho][Wo] window-local index, written by fwd(max) and consumed by bwd(max). */
int ssn_pool_fwd(int is_max, const float* x, float* y, unsigned char* argmax, int N, int C, int H, int W,
                 long x_img_stride, int Ho, int Wo, long y_img_stride, int ksize, int stride, int pad,
                 float* y_amax, hipStream_t stream);
int ssn_pool_bwd(int is_max, const float* dy, const unsigned char* argmax, float* dx, int N, int C, int H, int W,
                 long dx_img_stride, int Ho, int Wo, long dy_img_stride, int ksize, int stride, int pad,
                 int accumulate, const float* mask_y, long mask_img_stride, const float* mask_scale,
                 float* dx_amax, hipStream_t stream);
/* y = relu?(scale[c] * avgpool(x) + shift[c]) (average pools only): the pool-projection branch of an Inception block
 * (<block>_pool -> <block>_pool_proj + BN + ReLU) evaluated as avgpool(conv1x1(x)) -- identical to conv1x1(avgpool(x))
 * for zero padding with count_include_pad -- so that the pool touches the projection's output channels only. */
int ssn_avgpool_affine_fwd(const float* x, float* y, const float* scale, const float* shift, int relu, int N, int C,
                           int H, int W, long x_img_stride, int Ho, int Wo, long y_img_stride, int ksize, int stride,
                           int pad, float* y_amax, hipStream_t stream);
/* out[c] = sum_{n,hw} g[n][c][hw] (fixed order): bias gradient of such a projection (the gradient BEFORE the pool's
 * backward; the wgrad kernel's bias column sees the pooled gradient). */
int ssn_channel_sum(const float* g, float* out, int N, int C, int HW, long img_stride, void* workspace,
                    size_t ws_bytes, hipStream_t stream);   /* workspace: C * ssn_channel_sum_shares(N) floats */
int ssn_channel_sum_shares(int N);
int ssn_global_avgpool_fwd(const float* x, float* y, int N, int C, int HW, long x_img_stride, hipStream_t stream);
int ssn_global_avgpool_bwd(const float* dy, float* dx, int N, int C, int HW, long dx_img_stride, int accumulate,
                           float* dx_amax, hipStream_t stream);

/* nn.Dropout standing in for the backbone's `fc` (ssn_models.py:71-74). mask: uint8 per element.
 * counter (optional, int64[1] in device memory) is mixed into the Philox key and incremented by the
 * call, so a hipGraph replay draws a fresh mask each time. */
int ssn_dropout_fwd(const float* x, float* y, unsigned char* mask, long total, float p, unsigned long long seed,
                    long* counter, hipStream_t stream);
int ssn_dropout_bwd(const float* dy, const unsigned char* mask, float* dx, long total, float p,
                    hipStream_t stream);

/* ------------------------------------------------------------------ STPP
 * StructuredTemporalPyramidPooling.forward (ops/ssn_ops.py:39-70).  The part table carries the
 * reference's integer tick truncation (ops/ssn_ops.py:53-55), computed once on the host. */
#define SSN_STPP_MAX_PARTS 24
typedef struct SsnStppTable {
    int n_parts;
    int n_seg;
    int act_lo, act_hi;
    int lo[SSN_STPP_MAX_PARTS];
    int hi[SSN_STPP_MAX_PARTS];
    int norm[SSN_STPP_MAX_PARTS];
    int col[SSN_STPP_MAX_PARTS];
} SsnStppTable;
int ssn_stpp_fwd(const float* ft, const float* scaling, float* act_ft, float* stpp_ft, int P, int D,
                 const SsnStppTable* table, hipStream_t stream);
int ssn_stpp_bwd(const float* d_act, const float* d_stpp, const float* scaling, float* d_ft, int P, int D,
                 const SsnStppTable* table, hipStream_t stream);
/* The fused head of SSN.train_forward (ssn_models.py:268-289): STPP + activity / completeness / regression Linear + the prop_type
 * row selection as ONE launch each way (instead of 7 forward, 16 backward), same arithmetic and summation order as ssn_stpp_* /
 * ssn_linear_* / ssn_row_gather|scatter.  w / b / pos / idx / out / O / n: HOST arrays of 3 (activity, completeness, regression;
 * w[2] == NULL: no regression head); pos[h]: DEVICE int [P] = row of proposal p in head h's gathered output or -1; idx[h]: DEVICE
 * long [n_h] = proposal of gathered row r.  Forward: out[h] [n_h][O_h], act_ft [P][D], stpp_ft [P][m D] (kept for the backward).
 * Backward: dout[h] gradients of the gathered outputs -> d_ft [P n_seg][D], dw[h], db[h]. */
int ssn_heads_fwd(const float* ft, const float* scaling, const float* const* w, const float* const* b, const int* const* pos,
                  const long* const* idx, float* const* out, const int* O, const int* n, float* act_ft, float* stpp_ft, int P, int D,
                  const SsnStppTable* table, hipStream_t stream);
int ssn_heads_bwd(const float* ft_unused, const float* scaling, const float* const* w, const float* const* b, const int* const* pos,
                  const long* const* idx, float* const* dout, const int* O, const int* n, float* act_ft, float* stpp_ft, int P, int D,
                  const SsnStppTable* table, float* d_ft, float* const* dw, float* const* db, hipStream_t stream);
/* STPPReorgainzed.forward (ops/ssn_ops.py:109-170), stand-alone activity classifier form.
 * ranges: int32 [P][n_parts][2] row ranges (pr<=pl: skipped); act_range: int32 [P][2]. */
int ssn_stpp_reorg(const float* scores, int T, int D, const int* ranges, const int* act_range,
                   const float* scaling, const int* part_scale_col, int P, int n_parts, int act_len, int comp_len,
                   int reg_len, float* out_act, float* out_comp, float* out_reg, hipStream_t stream);

/* Dense testing (ssn_test.py:84-90): mean over the crops of the per-frame rows, `rst.view(num_crop, -1, D).mean(0)`
 * (x [num_crop][T][D] -> y [T][D]); and the regression de-normalisation reg[..., k] = reg[..., k] * std[k] + mean[k]
 * on reg [n_pairs][2], in place. */
int ssn_crop_mean(const float* x, float* y, int num_crop, int T, int D, hipStream_t stream);
int ssn_reg_denorm(float* reg, long n_pairs, float mean0, float std0, float mean1, float std1, hipStream_t stream);

/* RGBDiff input (SSN._get_diff, ssn_models.py:302-316, keep_rgb = False): in [n_segments][new_length + 1][C][HW] ->
 * out [n_segments][new_length][C][HW], out[g][x] = in[g][x + 1] - in[g][x]. */
int ssn_frame_diff(const float* in, float* out, long n_segments, int new_length, int C, int HW, hipStream_t stream);

/* Input side (csrc/frames.hip): the arithmetic of the reference's transform chain after decoding / scaling --
 * GroupOverSample or crop + horizontal flip, Stack(roll), ToTorchFormatTensor(div=False), GroupNormalize
 * (transforms.py:103-132, 49-64, 256-288, 67-80) -- on decoded uint8 frames.
 * src [n_img][Hs][Ws][C] uint8 HWC -> dst [n_crops][n_img][C][crop_h][crop_w] fp32; crop k is (off_x, off_y, flip);
 * roll: reverse the channel order (RGB -> BGR, Stack(roll=True)); invert_even: 255 - px on the even images of
 * flipped crops (flow x component); mean / stdv (DEVICE arrays of n_mean / n_std floats) repeat over the stacked
 * channels like GroupNormalize. */
int ssn_frames_crop_normalize(const unsigned char* src, float* dst, int n_img, int Hs, int Ws, int C, int crop_h,
                              int crop_w, int n_crops, const int* off_x, const int* off_y, const int* flip, int roll,
                              int invert_even, const float* mean, int n_mean, const float* stdv, int n_std,
                              hipStream_t stream);
/* The TRAINING chain on the GPU: GroupMultiScaleCrop (crop + PIL's bilinear resize to the network input: transforms.py:135-206,
 * restated bit-exactly from Pillow's 8-bit ImagingResample) -> GroupRandomHorizontalFlip (:49-64) -> Stack(roll) ->
 * ToTorchFormatTensor(div=False) -> GroupNormalize, i.e. SSN.get_augmentation() + the tail of ssn_train.py:106-111, on decoded
 * uint8 frames: the loader workers only decode.  src [n_img][Hs][Ws][C] uint8 -> dst [n_img][C][out_h][out_w] fp32; box: DEVICE int
 * [n_img][4] = (x0, y0, crop_w, crop_h) per image (one box per group in the reference), flip: DEVICE int [n_img]; the caller checks
 * that boxes lie inside the frame and crop / output <= 3 per axis.  workspace: ssn_frames_resize_workspace_bytes() device bytes. */
size_t ssn_frames_resize_workspace_bytes(int n_img, int out_h, int out_w);
int ssn_frames_crop_resize_normalize(const unsigned char* src, float* dst, int n_img, int Hs, int Ws, int C, int out_h, int out_w,
                                     const int* box, const int* flip, int roll, int invert_even, const float* mean, int n_mean,
                                     const float* stdv, int n_std, void* workspace, size_t workspace_bytes, hipStream_t stream);
/* The TEST-time GroupScale on the GPU (transforms.py:83-96; inside GroupOverSample :103-132 and in front of GroupCenterCrop,
 * ssn_test.py:107-115): Pillow's 8-bit BILINEAR resize of whole frames, bit-identical to img.resize((out_w, out_h), Image.BILINEAR).
 * src [n_img][Hs][Ws][C] uint8 -> dst [n_img][out_h][out_w][C] uint8, C = 1 or 3; the images of a call share one size (the frames of
 * one video), so there is one coefficient table per call.  Up to 13 taps per axis: the axis with the smaller in / out ratio (the
 * side GroupScale sets) may shrink by up to 6, the other one (its length is truncated to an integer) by less than 6.5.
 * workspace: ssn_frames_scale_workspace_bytes() device bytes, 4-byte aligned.  Two launches on `stream`, no allocation, no host read. */
size_t ssn_frames_scale_workspace_bytes(int out_h, int out_w);
int ssn_frames_scale(const unsigned char* src, unsigned char* dst, int n_img, int Hs, int Ws, int C, int out_h, int out_w,
                     void* workspace, size_t workspace_bytes, hipStream_t stream);

/* Detection post-processing of one video (csrc/detect.hip): score fusion softmax(activity)[1:] * exp(completeness),
 * top-k over all (proposal, class) pairs, temporal NMS per class and location regression
 * (eval_detection_results.py:91-128, 167-178; ops/utils.py:56-82).  act [P][C+1], comp [P][C], reg [P][C][2] or NULL
 * (fp32); rel_prop [P][2] fp64 normalised spans; combined [P][C] fp32 out; dets [C][max_det][5] fp64 = (start, end,
 * score, loc, dur) in descending score order, counts [C] int32; workspace: ssn_detections_workspace_bytes(P, C) bytes
 * of device scratch.  include_bg 1: softmax over all C+1 activity scores (the reference's top_k <= 0 branch) instead of
 * the C class scores (0); 2: no softmax, raw class scores (the --cls_scores branch without --softmax_before_filter, :135); top_k <= 0 keeps every pair, otherwise EXACTLY top_k pairs are kept as np.argsort(...)[-top_k:]
 * does (ties at the k-th score: the higher flat indices, i.e. a stable sort's choice).  Score ties inside a class:
 * higher proposal index first (scores.argsort()[::-1] of a stable sort).  Non-finite scores are ordered as numpy
 * orders them (NaN above +inf) and can never cause an out-of-range access.  Any P is accepted (P > 2048 sorts in the
 * workspace instead of LDS). */
size_t ssn_detections_workspace_bytes(int P, int C);
int ssn_detections(const float* act, const float* comp, const float* reg, const double* rel_prop, float* combined,
                   double* dets, int* counts, void* workspace, size_t ws_bytes, int P, int C, int max_det, int top_k,
                   int include_bg, double nms_thresh, int regress, hipStream_t stream);
/* The same for a BATCH of videos (csrc/detect_batch.hip): what eval_detection_results.py:91-178 runs video by video (the loop
 * at :146-160 over the score dict) in a number of launches that does not depend on V, bit-identical to ssn_detections per
 * video, ending in the flat rows ravel_detections (:188) forms.  The videos stand one after the other: act [total_p][C+1],
 * comp [total_p][C], reg [total_p][C][2] or NULL (fp32), rel_prop [total_p][2] fp64, p_off [V + 1] int32 (given twice: a
 * host copy that is validated before any launch, and the device copy the kernels read); report [V][C] uint8 or NULL: the
 * classes a video reports (the --cls_scores branch, :130-144); a pair whose byte is 0 does no work and has no rows.  top_k and
 * include_bg as above, top_k per video with flat indices counted inside the video.  total_p * C < 2^31.
 *   batch       combined [total_p][C] fp32; kept [total_p * C] int32: the surviving proposals (index inside the video) of class
 *               c of video v from p_off[v] * C + c * P_v on, in kept order; counts [V * C] int32; row_off [V * C + 1] int32 =
 *               exclusive prefix sums of counts.  A video with P_v > 2048 sorts in the workspace: big_off [V + 1] int64
 *               (device) = exclusive prefix sums of C * pow2(P_v) over those videos (nothing for the others), big_entries its
 *               last entry; workspace: ssn_detections_batch_workspace_bytes(V, big_entries) bytes, 16-byte aligned.
 *   batch_fill  after the caller's ONE host read, N = row_off[V * C]: rows [N][5] fp64 = (start, end, score, loc, dur), the
 *               values ssn_detections writes into dets, and cls / vid / prop [N] int32 (prop: index inside the video), in the
 *               order video, class ascending, kept order (descending score).
 * The kernels bound every index they derive from the device tables. */
size_t ssn_detections_batch_workspace_bytes(int V, long big_entries);
int ssn_detections_batch(const float* act, const float* comp, const double* rel_prop, const int* h_p_off, const int* d_p_off,
                         const unsigned char* report, const long* big_off, long big_entries, int V, int C, int top_k,
                         int include_bg, double nms_thresh, float* combined, int* kept, int* counts, int* row_off,
                         void* workspace, size_t ws_bytes, hipStream_t stream);
int ssn_detections_batch_fill(const double* rel_prop, const float* combined, const float* reg, const int* p_off, const int* kept,
                              const int* row_off, int V, int C, long total_p, long N, int regress, double* rows, int* cls,
                              int* vid, int* prop, hipStream_t stream);

/* Temporal actionness grouping for a BATCH of videos (csrc/tag.hip): gen_prop of gen_bottom_up_proposals.py:116-142, i.e.
 * label_frame_by_threshold (ops/sequence_funcs.py:11-34: fp32 softmax, scipy's gaussian_filter in fp64 with `reflect`
 * borders, one label row per threshold), build_box_by_search (:101-136), temporal_nms_fallback (:71-97, the `+ 1` form) and
 * the frames -> seconds conversion with the minimum-length mask (:138-141).  scores [total_T][2] fp32 = the videos'
 * actionness scores one after the other, offsets [V + 1] int32 frame offsets (given twice: a host copy that is validated
 * before any launch, and the device copy the kernels read), thresholds [n_thr] fp32, tolerances [n_tol] fp64, durations
 * [V] fp64 seconds (device).  Two phases with ONE host read between them, whatever V is:
 *   count:    prob / smoothed [total_T] fp32, labels [n_thr][total_T] uint8 (or NULL), runs [V][n_thr] int32 = foreground
 *             runs of every label row; the caller forms run_off [V * n_thr + 1] (exclusive prefix sums, int32) and
 *             sort_off [V + 1] int64 (pow2(candidates) sort entries for every video with more candidates than
 *             the LDS capacity the library reports, none for the others) and sizes the outputs from them;
 *   generate: row r emits 2 * n_tol * runs[r] candidates from 2 * n_tol * run_off[r] on, in the reference's order
 *             (cand_box [C][2] int32, cand_score [C] fp32: sequential fp32 sums, bit-equal to Python's sum()); per video
 *             the survivors of the NMS from its candidate base on (kept_box, kept_score, seconds [C][2] fp64, longer [C]
 *             uint8 = span > minimum_len) and kept_count [V].  Equal scores: smaller start, then smaller end, first.
 * Only the counting phase takes (and validates) a host copy of the offsets; the generating phase follows it on the same
 * device offsets, and its kernels bound every index they derive from the device tables.  total_T < 2^30.
 * Non-finite scores are ordered as numpy orders them and can never cause an out-of-range access. */
int ssn_tag_lds_candidates(void);
size_t ssn_tag_workspace_bytes(long total_runs, long sort_entries);
int ssn_tag_count(const float* scores, const int* h_offsets, const int* d_offsets, int V, int total_T,
                  const float* thresholds, int n_thr, double bw, float* prob, float* smoothed, unsigned char* labels,
                  int* runs, hipStream_t stream);
int ssn_tag_generate(const float* scores, const float* smoothed, const int* d_offsets, const double* durations, int V,
                     int total_T, const float* thresholds, int n_thr, const double* tolerances, int n_tol,
                     const int* run_off, const long* sort_off, long total_runs, long sort_entries, double nms_thresh,
                     double minimum_len, int* cand_box, float* cand_score, int* kept_box, float* kept_score,
                     double* seconds, unsigned char* longer, int* kept_count, void* workspace, size_t ws_bytes,
                     hipStream_t stream);
/* name_proposal (ops/detection_metrics.py:54-76) for a batch: ground truth gt_span [G][2] fp64 + gt_label [G] int32 ragged
 * by gt_off [V + 1], proposals prop [P][2] fp64 ragged by prop_off [V + 1] (all device) -> per proposal the label + 1 of
 * the instance with the largest temporal IoU (first maximum, IoU > thresh; else 0), that IoU and overlap / own length. */
int ssn_tag_name_proposals(const double* gt_span, const int* gt_label, const int* gt_off, int G, const double* prop,
                           const int* prop_off, int V, int P, double thresh, int* out_label, double* out_iou,
                           double* out_self, hipStream_t stream);

/* Detection evaluation of a whole dataset (csrc/eval.hip): the stage of eval_detection_results.py between ravel_detections
 * (:188) and the mean over classes (:237).  The AP function the reference calls there (:14, :220) belongs to the ActivityNet
 * toolkit, a submodule that is empty in the reference tree; the algorithm is restated in DESIGN.md.  Predictions of all
 * classes and videos flat in any order: pred_seg [N][2], pred_score [N] fp64, pred_cls / pred_vid [N] int32.  Ground truth
 * (get_all_gt, :200-203): gt_seg [G][2] fp64 with the rows of one (class, video) group next to each other in their input
 * order, groups [NG][5] int32 = (class, video, first row, rows, offset of the group's scratch in 8-byte units), npos [C]
 * int32 rows per class.  thresholds [T] fp64 (:209-212), T <= 32.  Two phases with ONE host read between them:
 *   count: counts [C + 1] int32 = predictions per class, counts[C] = rows with a class outside [0, C) or a score that is
 *          not finite (the caller refuses those); the caller forms pred_off [C + 1] int32 (exclusive prefix sums) and
 *          sort_off [C + 1] int64 (the same with every class rounded up to a power of two, 0 stays 0);
 *   ap:    order [N] int32 = flat indices class by class in descending score, equal scores lower flat index first; tp
 *          [T][N] uint8 in that order; ap [C][T] fp64, NaN for a class without ground truth.  Among ground-truth rows of
 *          equal IoU the earlier row is matched.  IoU = inter / ((ge - gs) + (e - s) - inter) in fp64, in that order.
 * A group with more rows than the LDS capacity the library reports takes rows + 32 * ceil(rows / 64) units of scratch
 * (`big_units` in total).  The kernels bound every index they derive from the device tables. */
int ssn_eval_lds_gt(void);
size_t ssn_eval_workspace_bytes(long sort_entries, long big_units, int C);
int ssn_eval_count(const double* pred_score, const int* pred_cls, int N, int C, int* counts, hipStream_t stream);
int ssn_eval_ap(const double* pred_seg, const double* pred_score, const int* pred_cls, const int* pred_vid, int N,
                const double* gt_seg, const int* groups, int NG, int G, const int* npos, const double* thresholds, int T, int C,
                const int* pred_off, const long* sort_off, long sort_entries, long big_units, int* order, unsigned char* tp,
                double* ap, void* workspace, size_t ws_bytes, hipStream_t stream);
/* temporal_recall (ops/detection_metrics.py:31-51, with temporal_iou :7-20: intersection over the hull) for a batch: gt_span
 * [G][2] fp64 ragged by gt_off [V + 1], prop [P][2] fp64 ragged by prop_off [V + 1], thresholds [T] fp64 (all device) -> hits
 * [V][T] int32: ground-truth spans of video v that some proposal overlaps with an IoU strictly above threshold t. */
int ssn_eval_recall(const double* gt_span, const int* gt_off, int G, const double* prop, const int* prop_off, int P, int V,
                    const double* thresholds, int T, int* hits, hipStream_t stream);

/* The proposal-list stage for a batch of videos (csrc/proposal_list.hip); naming and recall run on the two entries above,
 * on the device tensors these write.  fp64 / int32 only, every fp64 result one IEEE operation.
 *   sw_count / sw_fill   gen_exponential_sw_proposal (ops/sequence_funcs.py:37-54; called at gen_sliding_window_proposals.py:46):
 *                        level l has windows (k * step_l, k * step_l + span_l), k < ceil(duration / step_l) (the entries of
 *                        np.arange(0, duration, step_l)), kept while min(duration, start + span_l) - start >= 1 -- a prefix
 *                        in k.  durations [V] fp64 (device); h_spans / h_steps [L] int32 on the HOST (span_l = 2^l, step_l =
 *                        int(ceil(span_l * time_step * (1 - overlap))), both >= 1, L <= 31; validated before any launch).
 *                        Two phases with ONE host read between them: counts [V][L] int32, from which the caller forms
 *                        offsets [V * L + 1] int32 (exclusive prefix sums, total W < 2^30); then windows [W][2] fp64 in the
 *                        reference's order (per video: level ascending, start ascending).
 *   proposal_list_rows   the frame-number columns of dump_window_list (ops/io.py:109-127; called at
 *                        gen_sliding_window_proposals.py:62 and gen_bottom_up_proposals.py:185): per video real_fps =
 *                        double(frame_cnt) / duration, every span (s, e) of gt_span [G][2] (ragged by gt_off [V + 1]) and of
 *                        prop [P][2] (ragged by prop_off [V + 1]) becomes (int(s * real_fps), int(e * real_fps)), truncated
 *                        toward zero: gt_frames [G][2], frames [P][2] int32.  A product that is not finite or does not fit
 *                        int32 is written as 0 and sets bit 0 (ground truth) or bit 1 (proposal) of its video's word in
 *                        status [V] int32; other videos are unaffected.  All pointers device memory. */
int ssn_sw_count(const double* durations, int V, const int* h_spans, const int* h_steps, int L, int* counts,
                 hipStream_t stream);
int ssn_sw_fill(const int* offsets, int V, const int* h_spans, const int* h_steps, int L, int W, double* windows,
                hipStream_t stream);
int ssn_proposal_list_rows(const double* gt_span, const int* gt_off, int G, const double* prop, const int* prop_off, int P,
                           const int* frame_cnt, const double* durations, int V, int* gt_frames, int* frames, int* status,
                           hipStream_t stream);

/* The text of the list file, formed on the device (csrc/proposal_text.hip): dump_window_list (ops/io.py:95-134) under the
 * '# <index>' lines of the proposal scripts, byte for byte.  Inputs are the arrays the entries above left on the device:
 * gt_label [G] int32 AS WRITTEN (label + 1), gt_frames [G][2], gt_off [V + 1]; label [P], iou / own [P] fp64, frames
 * [P][2], prop_off [V + 1]; frame_cnt [V]; and the records to write: write [n_written] int32 (the video of record k),
 * paths: the UTF-8 bytes of the records' paths back to back, path_off [n_written + 1] int32 into them (path_bytes in all,
 * below 2^30), item_off [n_written + 1] int32: exclusive prefix sums of 3 + n_gt + K over the records (n_items in all).
 * Record k is
 *     # <first_index + k>\n<path>\n<frame_cnt>\n1\n<n_gt>\n   then   <label> <start> <end>\n   per ground-truth row,
 *     <K>\n   then   <label> <iou:.4f> <own:.4f> <start> <end>\n   per proposal row; a record without proposals ends 0\n\n.
 * Any int32 prints as C's %d; any finite double with |x| < 2^32 as C's %.4f (correctly rounded, ties to even, the sign
 * of -0.0 kept; integer arithmetic).  NaN, +-inf and |x| >= 2^32 print as ?.???? and set bit 2 of the video's word in
 * status [V] (ORed: the caller zeroes it or passes the status of ssn_proposal_list_rows).
 *   size   bp [ceil(n_items / 256) + 1] int32: exclusive prefix sums of the bytes of every 256 items and, last, the bytes of
 *          the text (-1: 2^31 or more).  ONE host read of that word sizes the output.
 *   fill   out [out_bytes] uint8 (any alignment; nothing is written at or behind out_bytes), rec_off [n_written + 1] int32:
 *          the first byte of every record and the end of the text.
 * Three launches whatever V is; no atomic decides a position; rows, videos and path ranges the tables do not cover are
 * left out.  All pointers device memory. */
int ssn_proposal_text_size(const int* gt_label, const int* gt_frames, const int* gt_off, int G, const int* label,
                           const double* iou, const double* own, const int* frames, const int* prop_off, int P,
                           const int* frame_cnt, int V, const int* path_off, long path_bytes, const int* write,
                           const int* item_off, int n_written, int n_items, int first_index, int* bp, int* status,
                           hipStream_t stream);
int ssn_proposal_text_fill(const int* gt_label, const int* gt_frames, const int* gt_off, int G, const int* label,
                           const double* iou, const double* own, const int* frames, const int* prop_off, int P,
                           const int* frame_cnt, int V, const unsigned char* paths, const int* path_off, long path_bytes,
                           const int* write, const int* item_off, int n_written, int n_items, int first_index, const int* bp,
                           unsigned char* out, long out_bytes, int* rec_off, hipStream_t stream);

/* The test table of a batch of videos (csrc/test_table.hip): from the frame-number columns of a proposal list to what the
 * dense tester needs per proposal -- the rows ProposalSampler.test_ticks forms (ssn_dataset.py:393-428) and the row ranges
 * STPPReorgainzed computes from them (ops/ssn_ops.py:125-157), for all videos at once.  frames [P][2] int32 (start, end),
 * ragged by p_off [V + 1] int32; frame_cnt [V] and n_rows [V] int32 (n_rows: the ticks of the video, len(arange(0,
 * frame_cnt - new_length, test_interval)), formed by the caller; the caller refuses frame_cnt < 2 and n_rows < 1).
 *   mark   keep [P] int32: end > start and start < frame_cnt (the two filters of a list record); pre [P] and bp
 *          [ceil(P / 256) + 1] int32: prefix sums of keep inside blocks of 256 rows and over the blocks; counts [V] int32:
 *          rows of the video in the table = kept proposals, 1 when there is none (the whole-video row (0, frame_cnt - 1)),
 *          -1 when the video holds a negative frame number.  ONE host read of counts sizes the table: k_off [V + 1] int32
 *          are their exclusive prefix sums, K the total.
 *   fill   the kept rows compacted in input order: src [K] int32 (index inside the video's input, -1: whole-video row),
 *          rel [K][2] fp64 (start / frame_cnt, min(end, frame_cnt) / frame_cnt), ticks [K][4] int32 and scaling [K][2] fp64
 *          as test_ticks forms them (every expression one fp64 operation, truncation toward zero), ranges [K][n_parts][2]
 *          and act [K][2] int32 as STPPReorgainzed.forward hands them to ssn_stpp_reorg: (0, 0) a skipped part, ends cut
 *          at n_rows, (-1, -1) a range that starts at or behind n_rows.  The STPP configuration comes from the HOST:
 *          h_stage_entries [3] pyramid levels per stage, h_parts [n_entries] parts per level, at most 16 parts in total.
 * Launches do not depend on V; no atomic decides a position (two runs write the same bytes); every index derived from a
 * device table is bounded.  All pointers but h_stage_entries / h_parts are device memory. */
int ssn_test_table_mark(const int* frames, const int* p_off, int P, const int* frame_cnt, int V, int* keep, int* pre, int* bp,
                        int* counts, hipStream_t stream);
int ssn_test_table_fill(const int* frames, const int* p_off, int P, const int* frame_cnt, const int* n_rows, int V,
                        const int* keep, const int* pre, const int* bp, const int* k_off, int K, const int* h_stage_entries,
                        const int* h_parts, int n_entries, int* src, double* rel, int* ticks, double* scaling, int* ranges,
                        int* act, hipStream_t stream);

/* Proposal evaluation of a batch of videos (csrc/proposal_eval.hip): average recall against the average number of
 * proposals per video (AR-AN), its area under the curve and recall against tIoU -- the ActivityNet toolkit's
 * average_recall_vs_avg_nr_proposals, restated in DESIGN.md (the toolkit is the empty submodule named above).  The flat
 * inputs are those of ssn_eval_recall; the proposals of a video are in rank order, best first, or `order` [P] int32 names
 * them in that order (rank r of video v is row order[prop_off[v] + r]).  The host derives from the per-video counts alone
 *   nr [V] int32    proposals of the video that exist after the truncation to max_avg_nr_proposals (0 without ground truth),
 *   pcn [J] fp64    the ascending fractions of the curve points: at point j video v shows min(int(nr[v] * pcn[j]), nr[v]),
 *   per_video       double(sum nr) / number of videos with ground truth.
 *   rank    score [P] fp64 (finite; the caller checks), sort_off [V + 1] int64 = exclusive prefix sums of the videos'
 *           proposal counts rounded up to a power of two (0 stays 0) -> order: per video descending score, equal scores
 *           lower flat index first (the rule of ssn_eval_ap).  A video of up to 2048 proposals is sorted in LDS.
 *   ar_an   first_hit [G][T] int32 = smallest rank r < nr[v] with tIoU(row, proposal) >= thresholds[t], -1 when none;
 *           tIoU = inter / ((ge - gs) + (e - s) - inter) in fp64 in that order, as ssn_eval_ap.  matches [T][J] int32 =
 *           rows whose first hit is shown at point j.  curves [T * J + 2 J + 1] fp64 = recall [T][J] (matches / G),
 *           avg_recall [J] (mean over t), proposals_per_video [J] (pcn[j] * per_video), auc (trapezoid of avg_recall over
 *           proposals_per_video, divided by its last entry).  A memset and two launches whatever V, G, P.
 * T <= 32, J <= ssn_proposal_eval_max_points() (4096), G >= 1; refused on the host before any launch otherwise.  All
 * pointers but the sizes are device memory; the kernels bound every index they derive from the device tables. */
int ssn_proposal_eval_max_points(void);
size_t ssn_proposal_eval_workspace_bytes(long sort_entries);
int ssn_proposal_eval_rank(const double* score, const int* prop_off, int P, int V, const long* sort_off, long sort_entries,
                           int* order, void* workspace, size_t ws_bytes, hipStream_t stream);
int ssn_proposal_eval_ar_an(const double* gt_span, const int* gt_off, int G, const double* prop, const int* prop_off, int P,
                            int V, const int* nr, const int* order, const double* thresholds, int T, const double* pcn, int J,
                            double per_video, int* first_hit, int* matches, double* curves, hipStream_t stream);

/* Video-level classification (csrc/video_cls.hip): the aggregation functions of ops/video_funcs.py and the metrics of
 * ops/metrics.py for a whole batch.  Rows of all videos one after the other, [N][C] fp32, ragged by offsets [V + 1] int32;
 * every pointer but the sizes is device memory and no call's launches depend on V.
 *   status       status [V] int32: 1 a non-finite value among the video's rows (x [N][width]), 2 no rows.
 *   crop_reduce  raw [N][crops][C] -> frm [N][C]: crops added in order and divided once, or (use_max) their maximum.
 *   window_max   window i of (video v, span s) covers ticks [i * steps[s], min(i * steps[s] + spans[s], T_v)); its per-class
 *                maxima go to row win_off[v * S + s] + i of out [W][C]; win_off [V * S + 1]: prefix sums of ceil(T_v / steps[s]).
 *   topk_mean    out [G][C]: per class the mean of the min(ks[g], n_g) largest of the rows seg_off[g] ... seg_off[g + 1], exact
 *                in value with ties at the cut (k-th largest by a 32-pass threshold search on order-preserving keys); NaN
 *                for a segment without rows.  ks[g] >= n_g: a plain sum.
 *   tpp          frm [N][stages * C] -> out [V][C] = (1 / T) sum_t frm[t][k_t * C + c], k_t = int(t * (stages / T)) in fp64.
 *   finish       out [V][C] = term 0 + sum_s w[s - 1] * term s (w NULL: 1), term s of video v at in + v * stride_v + s *
 *                stride_s; `divide`: by S afterwards; status [V] (or NULL) non-zero: the row is NaN; `softmax`: along C.
 *   metrics      scores [V][C], gt [V][C] uint8, label [V] int32 or NULL, top_ks [K] -> counts [K + 3 C] int32 (hits, class
 *                hits / totals / predictions), ap [C] fp64 (tied scores form one threshold; NaN without a positive video),
 *                results [K + 2] fp64: hit rates (stable ranking: of equal scores the higher class index ranks higher),
 *                mean AP, mean class accuracy over the classes among labels or predictions (first argmax). */
int ssn_vcls_lds_rows(void);
size_t ssn_vcls_metrics_workspace_bytes(int V, int C);
int ssn_vcls_status(const float* x, const int* offsets, int V, int N, int width, int* status, hipStream_t stream);
int ssn_vcls_crop_reduce(const float* raw, float* frm, int N, int crops, int C, int use_max, hipStream_t stream);
int ssn_vcls_window_max(const float* frm, const int* offsets, const int* win_off, const int* spans, const int* steps, int V,
                        int S, int N, int C, int W, float* out, hipStream_t stream);
int ssn_vcls_topk_mean(const float* rows, const int* seg_off, const int* ks, int G, int N, int C, float* out,
                       hipStream_t stream);
int ssn_vcls_tpp(const float* frm, const int* offsets, int V, int N, int C, int stages, float* out, hipStream_t stream);
int ssn_vcls_finish(const float* in, const float* weights, const int* status, int V, int S, int C, long stride_v,
                    long stride_s, int divide, int softmax, float* out, hipStream_t stream);
int ssn_vcls_metrics(const float* scores, const unsigned char* gt, const int* label, const int* top_ks, int V, int C, int K,
                     int* counts, double* ap, double* results, void* workspace, size_t ws_bytes, hipStream_t stream);

/* The scoring tail of the actionness stage and the merge in front of TAG (csrc/actionness.hip).
 * fc: test_fc on the backbone output of one call (binary_test.py:89, binary_model.py:237-240; a cuBLAS GEMM in the reference).
 *   feat [num_crop * ticks][D] fp32 crop-major, w [C][D], b [C] or NULL -> raw_true [T][num_crop][C], the video's staging
 *   tensor in TRUE layout: the logits of feature row c * ticks + t go to raw_true[tick0 + t][c][:].  One wave per row,
 *   16-byte loads, a summation order that depends on D alone (a tick scores bit-identically in any batching); any C, any D.
 * group: binary_test.py:84,90-92 for one video.  ref_batch 0: raw = raw_true (raw may be the same buffer).  ref_batch g > 0:
 *   the rows the reference writes, whose view(-1, num_crop, D) reads a crop-major batch of g ticks (load_binary_score.py:265)
 *   as tick-major: with q = i / g, b = min(g, T - g q), r = (i - g q) * num_crop + j, raw[i][j] = raw_true[g q + r % b][r / b].
 *   mean [T][C] = the crop mean of raw as gen_bottom_up_proposals.py:78 takes it: slot 0, plus slots 1 .. num_crop - 1 in
 *   order, one division by float(num_crop); bit-equal to numpy's.
 * merge: the merging loop of gen_bottom_up_proposals.py:76-91 for V videos x S streams in one launch.  rows [total_rows][C]
 *   fp32 = the crop-averaged scores stream-major (stream s of video v: rows offsets[s * V + v] .. offsets[s * V + v + 1]),
 *   offsets [S * V + 1] int32, weights [S] fp32, out_offsets [V + 1] int32 (all device), out [out_rows][C].  A shorter stream
 *   truncates the sum (for the streams after it too), a longer one is read at int(x * (T_add / float(T))) in fp64; fp32
 *   multiply, then add.  The output lengths follow from the input lengths, which the caller knows.  Every index derived from
 *   the device tables is bounded against total_rows / out_rows: a video whose tables are inconsistent writes nothing. */
int ssn_actionness_fc(const float* feat, const float* w, const float* b, float* raw_true, int ticks, int num_crop, int C, int D,
                      int tick0, int T, hipStream_t stream);
int ssn_actionness_group(const float* raw_true, float* raw, float* mean, int T, int num_crop, int C, int ref_batch,
                         hipStream_t stream);
int ssn_actionness_merge(const float* rows, const int* offsets, const float* weights, const int* out_offsets, float* out, int S,
                         int V, int C, int total_rows, int out_rows, hipStream_t stream);

/* ------------------------------------------------------------------ heads
 * nn.Linear fwd/bwd for activity_fc / completeness_fc / regressor_fc / test_fc
 * (ssn_models.py:77-78,87,272-273,283,300; cuBLAS GEMMs in the reference). */
int ssn_linear_fwd(const float* x, const float* w, const float* b, float* out, int R, int O, int D,
                   hipStream_t stream);
int ssn_linear_bwd(const float* dout, const float* x, const float* w, float* dx, float* dw, float* db, int R,
                   int O, int D, int accumulate_dx, hipStream_t stream);
/* prop_type row selection (ssn_models.py:275-289). */
int ssn_row_gather(const float* src, const long* index, float* dst, int n_idx, int width, hipStream_t stream);
int ssn_row_scatter(const float* src, const long* index, float* dst, int n_idx, int n_rows, int width,
                    hipStream_t stream);

/* ------------------------------------------------------------------ losses
 * CrossEntropyLoss (ssn_train.py:133,210).  workspace: 2*R floats; the first R (lse) feed the bwd. */
int ssn_ce_loss_fwd(const float* logits, const long* target, float* loss, float* workspace, int R, int C,
                    hipStream_t stream);
int ssn_ce_loss_bwd(const float* logits, const long* target, const float* lse, const float* gout, float* dlogits,
                    int R, int C, hipStream_t stream);
/* CompletenessLoss + OHEMHingeLoss (ops/ssn_ops.py:173-239).  den = pos_cnt + neg_cnt as the
 * reference truncates it (ops/ssn_ops.py:236-239).  coef: R floats kept for bwd; workspace 2*R floats. */
int ssn_completeness_loss_fwd(const float* pred, const long* labels, float* loss, float* coef, float* workspace,
                              int R, int C, int group, int split, int keep_pos, int keep_neg, float den,
                              hipStream_t stream);
int ssn_completeness_loss_bwd(const long* labels, const float* coef, const float* gout, float* dpred, int R, int C,
                              float den, hipStream_t stream);
/* ClassWiseRegressionLoss (ops/ssn_ops.py:242-258).  diff: 2*n floats kept for bwd. */
int ssn_cw_smoothl1_fwd(const float* pred, const long* labels, const float* targets, float* loss, float* diff,
                        int n, int C, hipStream_t stream);
int ssn_cw_smoothl1_bwd(const long* labels, const float* diff, const float* gout, float* dpred, int n, int C,
                        hipStream_t stream);

/* [r6] The training objective of ssn_train.py:210-214 -- activity CE + w_comp * completeness + w_reg * regression -- in ONE launch
 * (the three losses above, same bodies and summation orders, then the mix) and ONE backward launch.  losses[4] = activity,
 * completeness, regression (0 without that head), total.  lse [Ra], coef [Rc], diff [2 n_reg] are kept for the backward; scratch:
 * max(2 Ra, 2 Rc) floats.  reg_pred == NULL (d_reg == NULL in the backward): no regression head (ssn_models.py:288-289). */
int ssn_total_loss_fwd(const float* act_logits, const long* act_target, int Ra, int Ca, const float* comp_pred,
                       const long* comp_labels, int Rc, int Cc, int group, int split, int keep_pos, int keep_neg, float den,
                       const float* reg_pred, const long* reg_labels, const float* reg_targets, int n_reg, int Cr, float w_comp,
                       float w_reg, float* losses, float* lse, float* coef, float* diff, float* scratch, hipStream_t stream);
int ssn_total_loss_bwd(const float* act_logits, const long* act_target, int Ra, int Ca, const long* comp_labels, int Rc, int Cc,
                       float den, const long* reg_labels, int n_reg, int Cr, float w_comp, float w_reg, const float* lse,
                       const float* coef, const float* diff, const float* gout, float* d_act, float* d_comp, float* d_reg,
                       hipStream_t stream);
/* The label / target bookkeeping of SSN.train_forward (ssn_models.py:275-289): target[idx0], target[idx1], target[idx2],
 * reg_target[idx2] in one launch (the reference: four index_select behind three nonzero()).  n2 == 0: no regression. */
int ssn_label_select(const long* target, const float* reg_target, const long* idx0, int n0, const long* idx1, int n1,
                     const long* idx2, int n2, long* out0, long* out1, long* out2, float* out_reg, hipStream_t stream);

/* [r6] Checksum of the parameters a cached derivative (packed weights, folded BatchNorm vectors of the inference cache,
 * planes_exec.py) was built from -- the reference re-reads its parameters in every forward (ssn_models.py:298), so a write through
 * `p.data` is seen at once; torch's version counters do not see it, the bits do.  table: device array of n_entries {const void* ptr;
 * long n_words}; slot: device uint64, 0 on entry.  expected == NULL: slot += checksum (recording).  Otherwise additionally
 * flag |= bit when slot != *expected, and slot <- 0. */
int ssn_param_checksum(const void* table, int n_entries, unsigned long long* slot, const unsigned long long* expected, int* flag,
                       int bit, hipStream_t stream);

/* ------------------------------------------------------------------ optimiser step
 * torch.optim.SGD(momentum, weight_decay) over one flat segment (ssn_train.py:141-144,252);
 * per-group lr_mult / decay_mult of ssn_models.py:240-251 are folded into lr / weight_decay. */
/* skip_flag (device int, may be NULL): read at launch time; non-zero = leave w and the momentum buffer untouched.  It is the word
 * ssn_pl_range_check raises when a tensor of the step left the range of its delayed scale: optimizer.step() (ssn_train.py:252) of a
 * flagged step becomes a no-op, so the host can repeat the step with fresh scales -- also from inside a hipGraph replay. */
int ssn_sgd_step(float* w, const float* grad, float* momentum_buf, long n, float lr, float momentum,
                 float weight_decay, float grad_scale, int first_step, const int* skip_flag, hipStream_t stream);
/* The same update for `count` tensors in ceil(count/48) launches; w / grad / momentum_buf / n / lr / weight_decay
 * are HOST arrays (of device pointers resp. scalars), one entry per tensor. */
int ssn_sgd_step_multi(int count, float* const* w, const float* const* grad, float* const* momentum_buf,
                       const long* n, const float* lr, const float* weight_decay, float momentum, float grad_scale,
                       int first_step, const int* skip_flag, hipStream_t stream);
/* clip_grad_norm support (ssn_train.py:245-249): out[0] (+)= sum(x^2); workspace >= 1024 floats. */
int ssn_sumsq(const float* x, long n, float* out, int accumulate, float* workspace, hipStream_t stream);
int ssn_scale(float* x, long n, const float* coef_dev, float coef, hipStream_t stream);
/* ------------------------------------------------------------------ the training step's bookkeeping (csrc/train_step.hip)
 * Meters, clipping and the optimizer of ssn_train.py:216-253 / binary_train.py:180-204 in a constant number of launches and without
 * a host read (capturable into a hipGraph).  No atomics: every sum has a fixed order.
 *
 * ssn_step_meters: AverageMeter.update of all meters of one step, one launch of one workgroup.  logits fp32, `rows` rows of `cols`
 * values row_stride (>= cols) elements apart; target int64 [rows]; losses device fp32 [n_losses], 0 <= n_losses <= 4.  state: device
 * double [(n_losses + 3) * 4 + 1] = per meter {sum, count, last_num, last_den} (val = last_num / last_den, avg = sum / count), then
 * the number of skipped calls.  Meters: the losses (n = loss_weight), top-1 accuracy over all rows (n = rows), over the even rows
 * ("FG", n = rows / 2), over the odd rows ("BG").  An accuracy is float(correct) * float(100.0 / n_rows) in fp32 -- accuracy() of
 * ssn_train.py:401-414 -- widened and accumulated in double.  Prediction of a row: its largest value, the lowest column among equals,
 * NaN above every number, the first NaN taken; a target outside [0, cols) is a miss.  skip_flag (device int, may be null) non-zero:
 * only the skipped counter changes (the convention of ssn_sgd_step_multi).  rows must be even and positive. */
int ssn_step_meters(const float* logits, long row_stride, const long* target, int rows, int cols, const float* losses, int n_losses,
                    double loss_weight, double* state, const int* skip_flag, hipStream_t stream);
/* ssn_sumsq_multi: 2-norm over `count` fp32 tensors (HOST arrays of device pointers / lengths; zero lengths allowed; 4-byte
 * alignment suffices) in ceil(count / 48) + 1 launches: one fp32 partial per 4096-element block in a fixed workspace slot, then one
 * workgroup sums the partials in double in a fixed order.  out[0] = sqrt(sum x^2) * pre_scale; out[1] = the factor the update
 * applies to the gradients: pre_scale * c when c = max_norm / (out[0] + 1e-6) < 1, else pre_scale (ssn_train.py:239-248 with
 * pre_scale = 1 / iter_size).  max_norm <= 0: no clipping.  A NaN norm leaves out[1] = pre_scale, as the reference's test does.
 * workspace: at least ssn_sumsq_multi_workspace_floats(count, n) floats. */
long ssn_sumsq_multi_workspace_floats(int count, const long* n);
int ssn_sumsq_multi(int count, const float* const* x, const long* n, float* workspace, long ws_floats, float pre_scale,
                    float max_norm, float* out, hipStream_t stream);
/* ssn_sgd_step_multi with grad_scale read from device memory (out + 1 of ssn_sumsq_multi): same update, same launches. */
int ssn_sgd_step_multi_dev(int count, float* const* w, const float* const* grad, float* const* momentum_buf, const long* n,
                           const float* lr, const float* weight_decay, float momentum, const float* grad_scale_dev,
                           int first_step, const int* skip_flag, hipStream_t stream);
/* Kernel launches the three entry points above have issued on the calling thread since the last reset (tests, profiling). */
long ssn_train_step_launches(int reset);
/* The stem (conv1_7x7_s2 of model_zoo.BNInception, behind ssn_models.py:266) on the split kernels through its space-to-depth
 * form: a k x k / stride-2 / pad (k-1)/2 convolution on C channels is a (k+1)/2-tap stride-1 convolution on the 4C channels
 * xs[(c*2+a)*2+b][h'][w'] = x[c][2h'+a][2w'+b], with 2 padding pixels in front and 1 behind (k = 7): forward =
 * ssn_conv_x6_fwd_rect(xs, pack_rect(ssn_s2d_weights(w)), 4, 4, pad 2, Ho = H/2), weight gradient = ssn_conv_wgrad_x6(ksize 4,
 * pad 2) followed by ssn_s2d_weights_bwd.  (3 input channels fill 3/16 of a split slab directly; 12 fill 12/16.) */
int ssn_space_to_depth2(const float* x, float* xs, int N, int C, int H, int W, float* xs_amax, hipStream_t stream);
int ssn_s2d_weights(const float* w, float* w2, int Cout, int C, int k, hipStream_t stream);
int ssn_s2d_weights_bwd(const float* dw2, float* dw, int Cout, int C, int k, hipStream_t stream);
/* dst[i] += src[i]: sums the conv-gradient buffers of the sub-batches when one backward is executed in chunks (a batch
 * whose activations exceed the 2 GiB a kernel operand can address; DataParallel's reduce of replica gradients). */
int ssn_add_inplace(float* dst, const float* src, long n, hipStream_t stream);
/* out[n][c][h][w] = h < Ho && w < Wo ? g[n][c][h][w] : 0 (planes H x W >= Ho x Wo): the output gradient of an UNPADDED
 * stride-1 convolution on its input's grid, which makes its weight gradient a same-grid problem with taps 0 .. k-1 behind
 * the pixel: ssn_conv_wgrad_x6_rect(kh, kw, pad 0, 0) on (out, x).  The values are g's: out shares g's amax slot. */
int ssn_embed_planes(const float* g, float* out, int N, int C, int Ho, int Wo, long g_img_stride, int H, int W,
                     long out_img_stride, hipStream_t stream);

/* ================================================================== planes tensors (ABI 5)
 * The MFMA-native activation format of the split-precision path (csrc/planes.h): an fp32 activation x of the backbone behind
 * /root/reference/ssn_models.py:266,298 is kept as TWO f16 terms of x * s -- hi = f16(x s), lo = f16(x s - hi), s a power of
 * two per tensor -- in the channel-blocked layout
 *     plane (hi | lo)  |  image n  |  channel group g = c / 8  |  pixel q  |  channel c % 8        (f16; 16 bytes per pixel & group)
 * produced by the kernel that computes x (conv / pool epilogues), so that no consumer converts operands in its inner loop.
 * Pointers `*_hi` / `*_lo` address the two planes at the first channel group of a channel slice (slices start at multiples of 8
 * channels), `*_img_groups` = channel groups (C / 8) of the whole tensor.  Scales are "delayed": `*_scale` points at the
 * tensor's scale slot, fixed while a step runs and derived from the magnitude recorded in the previous step;
 * `*_amax` at its amax slot, raised by every producer (ssn_pl_scales_update turns one into the other between steps and flags
 * tensors that outgrew their head-room).  Packed weights are those of ssn_conv_x6_pack_*. */
int ssn_pl_scales_update(float* amax, float* scale, int* flag, int n, int exact, int slot0, int odd_extra_bits, hipStream_t stream);
/* (slot0 = global index of the first of the n slots; slots with an ODD global index -- where the executor keeps its gradient tensors,
 * whose maxima move far more from step to step than an activation's -- get odd_extra_bits more bits of head-room.) */
/* The range guard of the delayed scales: one launch at the END of a forward / backward pass over the `n` slots of the executor.
 * flag[0] |= 1 if a tensor's recorded (pre-clamp) maximum did not fit the scale it was stored with (its values were clamped to the
 * f16 range), |= 2 if it fell more than 8 bits below the target range (precision draining).  Modifies no slot.  The reference has no
 * counterpart (cuDNN computes in fp32 storage); this is what lets loss.backward() / optimizer.step() (ssn_train.py:236,252) and the
 * alternating train / validate passes (ssn_train.py:191-253, 278-362) run on data whose magnitude changes from call to call: the
 * host repeats a flagged pass with fresh scales, ssn_sgd_step_multi(skip_flag) refuses to consume a flagged step's gradients. */
int ssn_pl_range_check(const float* amax, const float* scale, int* flag, int n, int odd_extra_bits, hipStream_t stream);
/* fp32 NCHW <-> planes (the caller's frames, test inputs, the fp32 feature boundary); s2d: the space-to-depth view of the stem. */
int ssn_pl_from_f32(const float* x, long x_img_stride, void* hi, void* lo, int N, int C, int H, int W, long img_groups, int s2d,
                    const float* scale, float* amax, hipStream_t stream);
/* im2col of a planes slice with few channels: y[n][c kh kw + r kw + s][ho][wo] = x[n][c][ho stride + r - pad_h][wo stride + s - pad_w]
 * (both planes copied, y carries x's scale): the weight gradient of a first convolution that is not run in space-to-depth form becomes a
 * 1x1 problem on C kh kw channels (cuDNN wgrad of the first layer behind ssn_train.py:236 for --arch InceptionV3). */
int ssn_pl_im2col(const void* x_hi, const void* x_lo, long x_img_groups, void* y_hi, void* y_lo, long y_img_groups, int N, int C, int H,
                  int W, int Ho, int Wo, int kh, int kw, int stride, int pad_h, int pad_w, hipStream_t stream);
int ssn_pl_to_f32(const void* hi, const void* lo, long img_groups, float* y, long y_img_stride, int N, int C, int HW,
                  const float* scale, hipStream_t stream);
/* conv + frozen-BN affine + ReLU (cuDNN conv / BN(eval) / ReLU behind ssn_models.py:266) on planes slices: any kh x kw taps,
 * stride 1 / 2; raw_from / row_split / row_gap as ssn_conv_x6_fwd (fused launch on an Inception block input).  tile_cfg < 0: the
 * heuristic; 0 .. ssn_conv_pl_tiles() - 1: that tile; 32 + c: the haloed kernel with tile c on 3x3 / stride 1 / pad 1 layers (each
 * input pixel is staged once per channel group instead of once per tap; ssn_conv_pl_halo_taken says whether the launch takes it,
 * a layer or tile it does not fit runs the plain kernel with tile c); 48 + c: the same with pixel tiles that do not cross images (the
 * 56 x 56 layer: a 128-pixel tile across two images does not fit the halo buffer; prepared in round 4, not yet measured). */
int ssn_conv_pl_fwd(const void* x_hi, const void* x_lo, const float* w_packed, const float* scale, const float* shift, void* y_hi,
                    void* y_lo, int N, int Cin, int H, int W, long x_img_groups, int Cout, int Ho, int Wo, long y_img_groups, int kh,
                    int kw, int stride, int pad_h, int pad_w, int relu, int tile_cfg, const float* x_scale, const float* y_scale,
                    float* y_amax, int raw_from, int row_split, int row_gap, hipStream_t stream);
/* data gradient (loss.backward(), ssn_train.py:236) of a stride-1 layer; mask_hi / mask_scale fuse the ReLU + frozen-BN backward
 * of the layer that produced the input (only the SIGN of its high plane is read); taps_reversed: pack mode 2 operand. */
int ssn_conv_pl_dgrad(const void* dy_hi, const void* dy_lo, const float* wt_packed, void* dx_hi, void* dx_lo, int N, int Cout,
                      int Ho, int Wo, long dy_img_groups, int Cin, int H, int W, long dx_img_groups, int kh, int kw, int pad_h,
                      int pad_w, int accumulate, const void* mask_hi, long mask_img_groups, const float* mask_scale, int tile_cfg,
                      const float* dy_scale, const float* dx_scale, float* dx_amax, int k_split, int k_gap, int taps_reversed,
                      hipStream_t stream);
/* ... of a 3x3 / stride-2 layer (pad 1 on an even input, or pad 0): four parity-class launches (ssn_conv_x6_pack_dgrad_s2). */
int ssn_conv_pl_dgrad_s2(const void* dy_hi, const void* dy_lo, const float* wt_packed, void* dx_hi, void* dx_lo, int N, int Cout,
                         int Ho, int Wo, long dy_img_groups, int Cin, int H, int W, long dx_img_groups, int pad, int accumulate,
                         const void* mask_hi, long mask_img_groups, const float* mask_scale, int tile_cfg, const float* dy_scale,
                         const float* dx_scale, float* dx_amax, hipStream_t stream);
/* weight + bias gradient (cuDNN wgrad behind ssn_train.py:236): the reduction index is the pixel, so the operands are read
 * with the LDS transpose read; tile_cfg >= 100 / < 0: the nine-tap kernel for 3x3 / stride 1 / pad 1 layers. */
int ssn_conv_wgrad_pl(const void* g_hi, const void* g_lo, const void* x_hi, const void* x_lo, float* dw, float* db, int N, int Cin,
                      int H, int W, long x_img_groups, int Cout, int Ho, int Wo, long g_img_groups, int kh, int kw, int stride,
                      int pad_h, int pad_w, void* workspace, long ws_bytes, int tile_cfg, const float* g_scale,
                      const float* x_scale, int g_row_split, int g_row_gap, int* deferred_reduce, hipStream_t stream);
/* deferred_reduce (HOST int[2], may be NULL): when given, the split-K slabs are left in `workspace` -- which then must stay untouched
 * until the caller has reduced them -- and {slabs, taps} for ssn_wgrad_reduce_multi are written there instead of launching the
 * reduction: a backward pass reduces the slabs of all its layers in one launch. */
int ssn_wgrad_reduce_multi(int count, const float* const* part, float* const* dw, float* const* db, const int* M, const int* K,
                           const int* splits, const int* taps, hipStream_t stream);
long ssn_conv_wgrad_pl_workspace_bytes(int N, int Cin, int Cout, int Ho, int Wo, int kh, int kw, int tile_cfg);
/* GROUPED weight gradients: every weight + bias gradient of a backward pass (all the cuDNN wgrad calls behind loss.backward(),
 * /root/reference/ssn_train.py:236) in at most five launches (one per kernel family that has problems) + one reduction.  Problem i takes the arguments of ssn_conv_wgrad_pl as
 * array entries (HOST arrays): plane pointers, dw[i], db[i] (may be NULL), scale pointers, shape[16 i ..] = {N, Cin, H, W, Cout, Ho,
 * Wo, kh, kw, stride, pad_h, pad_w, g_row_split, g_row_gap, tile hint, 0} (hint -1: chosen; 0 / 3 / 8: one-tap 64x64 / 128x128 /
 * 96x128; 100: nine taps; 200: chunked 1x1; 300: the 4x4-tap space-to-depth stem), groups[2 i ..] = {x_img_groups, g_img_groups}.  The problems travel in a device-resident
 * table (`table`: ssn_conv_wgrad_pl_group_table_bytes(count) bytes, written by the call); each kernel family runs ONE grid over all its
 * problems, items ordered longest first, the reduction ranges split only as far as the whole group needs; partial slabs
 * (`workspace`: ssn_conv_wgrad_pl_group_workspace_bytes bytes; plan_out, optional: [count][4] = family, variant, splits, units per
 * split) are reduced in a fixed order: deterministic.  Capturable, no host sync. */
int ssn_conv_wgrad_pl_group(int count, const void* const* g_hi, const void* const* g_lo, const void* const* x_hi,
                            const void* const* x_lo, float* const* dw, float* const* db, const int* shape, const long* groups,
                            const float* const* g_scale, const float* const* x_scale, void* workspace, long ws_bytes, void* table,
                            long table_bytes, hipStream_t stream);
/* shape[16 i + 15] > 0: units per split of problem i, given by the caller instead of planned -- a call that holds only PART of a
 * pass's problems passes what the plan of the whole pass (plan_out) gave them, so that its slabs are split, and summed, as in one
 * call.  The same call with (a) every family's slabs reduced right behind its kernel, the family with the most slab bytes first,
 * and (b) the families fanned out over n_lanes (<= 8) side streams of the caller: the table writes stay on `stream`, family k and
 * its reduction run on lanes[k % n_lanes], forked behind the table writes by an event (created once per device, no timing, never
 * inside a capture: a first call on a capturing stream keeps to `stream`).  join != 0: `stream` waits for every lane before the
 * call returns; join == 0: the lanes are left running and the CALLER joins them (a later call with join != 0 on the same lanes
 * does).  n_lanes == 0: one stream.  Bit-identical to ssn_conv_wgrad_pl_group.  Capturable, no host sync. */
int ssn_conv_wgrad_pl_group_lanes(int count, const void* const* g_hi, const void* const* g_lo, const void* const* x_hi,
                                  const void* const* x_lo, float* const* dw, float* const* db, const int* shape, const long* groups,
                                  const float* const* g_scale, const float* const* x_scale, void* workspace, long ws_bytes,
                                  void* table, long table_bytes, hipStream_t stream, const hipStream_t* lanes, int n_lanes, int join);
long ssn_conv_wgrad_pl_group_workspace_bytes(int count, const int* shape, const long* groups, int* plan_out);
long ssn_conv_wgrad_pl_group_table_bytes(int count);
void ssn_conv_wgrad_pl_group_tuning(double fixed_nine, double fixed_one, int min_units_nine, int min_units_one); /* tooling / tests: planner constants (<= 0: keep) */
int ssn_conv_wgrad_pl_tiles(void);
int ssn_conv_pl_tiles(void);
int ssn_conv_pl_halo_taken(int N, int H, int W, int tile_cfg);
int ssn_conv_pl_tile_shape(int cfg, int* bm, int* bn);
void ssn_conv_pl_debug_flags(int flags);                    /* tooling (tools/ablate_conv_pl.py) */
void ssn_conv_pl_debug_trace(unsigned long long* buf);
void ssn_conv_wgrad_pl_debug_trace(unsigned long long* buf); /* tooling (tools/trace_wgrad_pl.py) */
void ssn_conv_wgrad_pl_debug_flags(int flags);
/* nn.MaxPool2d(ceil_mode) of the backbone manifest forward / backward (uint8 window-local argmax, torch's tie rule; dx_f32:
 * write the input gradient as fp32 NCHW instead), the 3x3 average pool behind its 1x1 projection (+ affine + ReLU; without
 * affine: its backward stencil), the ReLU / frozen-BN backward of a slice, global average pool forward / backward, and the
 * per-channel sums that give a projection's bias gradient. */
int ssn_pl_maxpool_fwd(const void* x_hi, const void* x_lo, long x_img_groups, void* y_hi, void* y_lo, long y_img_groups,
                       unsigned char* argmax, int N, int C, int H, int W, int Ho, int Wo, int k, int s, int pad,
                       const float* x_scale, const float* y_scale, float* y_amax, hipStream_t stream);
int ssn_pl_maxpool_bwd(const void* dy_hi, const void* dy_lo, long dy_img_groups, const unsigned char* argmax, void* dx_hi,
                       void* dx_lo, long dx_img_groups, int N, int C, int H, int W, int Ho, int Wo, int k, int s, int pad,
                       int accumulate, const void* mask_hi, long mask_img_groups, const float* mask_scale, int mask_pooled,
                       const float* dy_scale, const float* dx_scale, float* dx_amax, float* dx_f32, long dx_f32_img_stride,
                       hipStream_t stream);      /* mask_pooled: mask_hi = hi plane of the pool's OUTPUT (3x3 / stride 2, no accumulation) */
int ssn_pl_avgpool_affine(const void* x_hi, const void* x_lo, long x_img_groups, void* y_hi, void* y_lo, long y_img_groups,
                          const float* scale, const float* shift, int relu, int N, int C, int H, int W, int k, int pad,
                          const float* x_scale, const float* y_scale, float* y_amax, hipStream_t stream);
int ssn_pl_relu_bn_bwd(void* g_hi, void* g_lo, long g_img_groups, const void* y_hi, long y_img_groups, const float* scale, int N,
                       int C, int HW, const float* g_scale, float* g_amax, hipStream_t stream);
int ssn_pl_gap_fwd(const void* x_hi, const void* x_lo, long x_img_groups, float* y, int N, int C, int HW, const float* x_scale,
                   hipStream_t stream);
int ssn_pl_gap_bwd(const float* dy, void* dx_hi, void* dx_lo, long dx_img_groups, int N, int C, int HW, const void* mask_hi,
                   long mask_img_groups, const float* mask_scale, const float* dx_scale, float* dx_amax, hipStream_t stream);
long ssn_pl_channel_sum_workspace_bytes(int C);
int ssn_pl_channel_sum(const void* g_hi, const void* g_lo, long g_img_groups, float* out, int N, int C, int HW,
                       const float* g_scale, void* workspace, long ws_bytes, hipStream_t stream);
/* count slices of one pass in ONE pair of launches (host arrays; the same N; workspace: ssn_pl_channel_sum_workspace_bytes(sum C));
 * per slice bit-identical to ssn_pl_channel_sum. */
int ssn_pl_channel_sum_multi(int count, const void* const* g_hi, const void* const* g_lo, const long* g_img_groups, float* const* out,
                             int N, const int* C, const int* HW, const float* const* g_scale, void* workspace, long ws_bytes,
                             hipStream_t stream);
/* training-mode BatchNorm2d (+ ReLU) on planes slices (csrc/planes_bn.hip): bn_mode 'partial' / 'full' of ssn_models.py:95-105,
 * 156-174 on the planes executor; the mathematics of ssn_bn_train_* above.  C a multiple of 8; z is the convolution output WITHOUT
 * its bias; mean / invstd / running statistics / dgamma / dbeta in real units.  bwd: y_hi = HIGH plane of the layer's output (the
 * ReLU decision; NULL: no ReLU); dz goes to the planes slice (dz_hi, dz_lo) or, with dz_f32, to an fp32 NCHW tensor. */
long ssn_pl_bn_train_workspace_bytes(int C);
int ssn_pl_bn_train_stats(const void* z_hi, const void* z_lo, long z_img_groups, const float* z_scale, const float* conv_bias,
                          float* mean, float* invstd, float* running_mean, float* running_var, int N, int C, int HW, float eps,
                          float momentum, void* workspace, long ws_bytes, hipStream_t stream);
int ssn_pl_bn_train_apply(const void* z_hi, const void* z_lo, long z_img_groups, const float* z_scale, void* y_hi, void* y_lo,
                          long y_img_groups, const float* y_scale, float* y_amax, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, int relu, int N, int C, int HW, hipStream_t stream);
int ssn_pl_bn_train_bwd(const void* dy_hi, const void* dy_lo, long dy_img_groups, const float* dy_scale, const void* y_hi,
                        long y_img_groups, const void* z_hi, const void* z_lo, long z_img_groups, const float* z_scale,
                        const float* mean, const float* invstd, const float* gamma, float* dgamma, float* dbeta, void* dz_hi,
                        void* dz_lo, long dz_img_groups, const float* dz_scale, float* dz_amax, float* dz_f32,
                        long dz_f32_img_stride, int N, int C, int HW, void* workspace, long ws_bytes, hipStream_t stream);

/* TV-L1 optical flow for the Flow modality (csrc/flow.hip): the stage the reference's README hands to dense_flow (OpenCV's CUDA
 * OpticalFlowDual_TVL1).  The algorithm, its parameters and the standing of its parity are in DESIGN.md section 3.9.  Images are
 * fp32 [B][H][W] gray in [0, 255]; a level's state is two buffers [B][6][H][W] (u1, u2, p11, p12, p21, p22) and the per-warp
 * constants cst [B][4][H][W] (gx, gy, grad, rho_c).  ctl is a per-pair record int32 [B][4] = {done, launches, iterations, 0}: the
 * pair's current state is in buffer (launches & 1); every call that takes ctl_in / ctl_out reads one slot and writes ANOTHER
 * (the caller alternates two), so that no workgroup reads a word that another workgroup of the same launch writes.  Nothing here
 * reads back to the host: the caller enqueues the worst-case number of launches and the workgroups of a finished pair exit.
 *  gray      (4899 R + 9617 G + 1868 B + 8192) >> 14 on uint8 [pixels][3].
 *  resize    bilinear, source coordinate (d + 0.5) * src / dst - 0.5, indices clamped; plane c of a batch element is multiplied by
 *            mul_x (c even) or mul_y (c odd).  With ctl, element b is read from src1 when its state is in buffer 1.
 *  warp      starts a warp: brings the pair's state to state0, samples I1 and its centred gradient at (x + u1, y + u2) clamped to
 *            the image, writes cst and a fresh record.  ctl_in NULL: the state is in state0 (first warp of a level).
 *  iterate   n_iter (1 .. halo) iterations of every pair that is not done.  part_in [B][tiles] or NULL: the error partials of
 *            the chunk the previous launch ended, summed in tile order and tested against err_thresh by every workgroup;
 *            part_out [B][tiles] or NULL: this launch ends a chunk and writes its last iteration's partials.  iters [B] follows
 *            the pair's iteration count.  tiles = ceil(H / th) * ceil(W / tw) of the tile shape below.
 *  quantize  dense_flow's CAST, in fp32: v > bound -> 255, v < -bound -> 0, else rintf(255 (v + bound) / (2 bound)). */
int ssn_tvl1_tile_shape(int* th, int* tw, int* halo);
int ssn_flow_gray(const unsigned char* rgb, unsigned char* gray, long pixels, hipStream_t stream);
int ssn_flow_resize(const float* src0, const float* src1, const int* ctl, float* dst, int B, int C, long src_bstride, long dst_bstride,
                    int Hs, int Ws, int Hd, int Wd, float mul_x, float mul_y, hipStream_t stream);
int ssn_tvl1_warp(const float* I0, const float* I1, float* state0, const float* state1, float* cst, const int* ctl_in, int* ctl_out,
                  int B, int H, int W, hipStream_t stream);
int ssn_tvl1_iterate(float* state0, float* state1, const float* cst, int B, int H, int W, int n_iter, float l_t, float theta,
                     float taut, float err_thresh, const int* ctl_in, int* ctl_out, const float* part_in, float* part_out, int* iters,
                     hipStream_t stream);
int ssn_flow_quantize(const float* flow, unsigned char* out, long n, float bound, hipStream_t stream);

/* Baseline JPEG decoding of a batch of files (csrc/jpeg.hip): what the reference's loader workers do with PIL in _load_image,
 * Image.open(path).convert('RGB') / .convert('L') (ssn_dataset.py:208-215), bit for bit (libjpeg's islow inverse DCT, fancy upsampling
 * and 16-bit colour conversion).  The host walks the markers (jpeg_decode.py) and describes the batch in
 * device tables: desc int32 [images][desc_ints], units int32 [units][unit_ints] (one row per restart interval or per scan, padded
 * with image = -1 to rows of 64), tables uint32 [sets][4][table_words] (the distinct Huffman table sets: per table 512 16-bit
 * first-level entries (length << 8 | symbol, 0: longer than 9 bits), maxcode[17], valoff[17], 256 symbols), quant uint16 [n][64] in
 * natural order.  A workgroup of the entropy stage stages at most lds_sets consecutive sets.
 *  layout    the four sizes above.
 *  entropy   replaces the Huffman decoding inside Image.open: zero-fills coef int16 [total_blocks][64] (natural order) and status
 *            int32 [images], then one lane per unit.  A unit that runs out of data (1), meets an undefined code (2), overruns a
 *            block (4) or has an unusable table row (8) ORs that bit into its image's status word and stops.
 *  idct      replaces libjpeg's dequantisation + jpeg_idct_islow: coef -> uint8 component planes padded to whole MCUs.
 *  pixels    replaces libjpeg's upsampling, YCbCr -> RGB conversion and PIL's .convert(mode): planes -> uint8 [H][W][out_c] per
 *            image at its output offset, out_c 3 (RGB) or 1 (L). */
int ssn_jpeg_layout(int* desc_ints, int* unit_ints, int* table_words, int* lds_sets);
int ssn_jpeg_entropy(const unsigned char* bits, long bits_bytes, const int* desc, int n_images, const int* units, int n_units,
                     const unsigned int* tables, int n_sets, short* coef, long total_blocks, int* status, hipStream_t stream);
int ssn_jpeg_idct(const short* coef, long total_blocks, const int* desc, int n_images, int max_blocks, const unsigned short* quant,
                  int n_quant, unsigned char* planes, long plane_bytes, hipStream_t stream);
int ssn_jpeg_pixels(const unsigned char* planes, long plane_bytes, const int* desc, int n_images, long max_pixels, int out_c,
                    unsigned char* out, long out_bytes, hipStream_t stream);

/* The restart-interval index of a batch on the device (csrc/jpeg.hip): replaces the marker search of jpeg_decode._parse_scan and the
 * per-unit loop of JpegDecoder._plan.  bits holds every file from the first byte of its entropy-coded data to the file's end, each
 * file's first byte at a multiple of 16; columns 15 .. 18 of a file's desc row say where: first byte, end byte, first unit row,
 * units its header promises (ceil(MCUs / restart interval), 1 without a DRI; 0: the file is not indexed).  The unit rows arrive with
 * everything the bytes do not decide (image, MCU range, table set, workgroup pair, padding rows).
 *  index         one workgroup per file, 16 bytes per lane: a marker is FF followed by neither 00 nor FF, the scan ends at the first
 *                marker that is not RST0..7 (or at the file's end), the k-th restart marker at p ends unit k at p and begins unit
 *                k + 1 at p + 2, units the data does not contain get (end, end).  Writes begin / end of the file's rows (only rows
 *                inside the table that name the file) and refused int32 [images]: 16 for more restart markers than the promised
 *                units allow, another SOS or a DNL behind the scan, or a desc row whose ranges had to be clamped; else 0.
 *  index_status  status[i] |= refused[i], after ssn_jpeg_entropy (which zeroes status). */
int ssn_jpeg_index(const unsigned char* bits, long bits_bytes, const int* desc, int n_images, int* units, int n_units, int* refused,
                   hipStream_t stream);
int ssn_jpeg_index_status(const int* refused, int* status, int n_images, hipStream_t stream);

/* Baseline JPEG encoding of a batch of images (csrc/jpeg_encode.hip): the bytes PIL's Image.save(f, "JPEG", quality=, subsampling=,
 * restart_marker_blocks=) writes, byte for byte, for the libjpeg PIL links.  The host (jpeg_encode.py) describes
 * the batch in desc int32 [images][desc_ints] and prepares the quantisation tables (uint16 [2][64], natural order), the Huffman code
 * tables (uint32 [4][256]: DC luma, AC luma, DC chroma, AC chroma, entry = length << 16 | code) and the header bytes of every file.
 *  blocks    colour conversion, edge expansion, downsampling, islow forward DCT, quantisation: pix uint8 ([H][W] or [H][W][3] per image
 *            at its offset) -> coef int16 [total_blocks][64], zigzag order, rows in the scan's MCU order, dummy blocks included.
 *  count     zero-fills status, then blkbits int32 [total_blocks]: the bits the Huffman codes of every block take.
 *  scan      blkbits -> the bit offset of every block in its restart interval; ivals int32 [total_intervals] -> the byte offset of every
 *            interval in its image's raw region; rawlen int32 [images] (0, and status bit 1, for an image past its raw capacity).
 *  pack      zero-fills raw [raw_bytes], then every block ORs its codes in at its bit offset; intervals end padded with 1-bits.
 *  assemble  ffcount int32 [images] (scratch), then lengths int32 / offsets int64 [images] and the files in data: header, scan with 00
 *            after every FF and RSTn between intervals, FFD9.  A file longer than its capacity gets length 0 and status bit 1.
 * status bits: 1 the file does not fit, 2 a coefficient the tables have no code for, 4 an unusable desc row. */
int ssn_jpeg_enc_layout(int* desc_ints, int* block_bits);
int ssn_jpeg_enc_blocks(const unsigned char* pix, long pix_bytes, const int* desc, int n_images, int max_blocks,
                        const unsigned short* quant, short* coef, long total_blocks, hipStream_t stream);
int ssn_jpeg_enc_count(const short* coef, long total_blocks, const int* desc, int n_images, int max_blocks, const unsigned int* tables,
                       int* blkbits, int* status, hipStream_t stream);
int ssn_jpeg_enc_scan(const int* desc, int n_images, int* blkbits, long total_blocks, int* ivals, long total_intervals, int* rawlen,
                      int* status, hipStream_t stream);
int ssn_jpeg_enc_pack(const short* coef, long total_blocks, const int* desc, int n_images, int max_blocks, const unsigned int* tables,
                      const int* blkbits, const int* ivals, long total_intervals, const int* rawlen, unsigned char* raw, long raw_bytes,
                      int* status, hipStream_t stream);
int ssn_jpeg_enc_assemble(const unsigned char* raw, long raw_bytes, const int* desc, int n_images, const int* ivals, long total_intervals,
                          const int* rawlen, const unsigned char* headers, long header_bytes, int* ffcount, unsigned char* data,
                          long data_bytes, long* offsets, int* lengths, int* status, hipStream_t stream);

/* Lossless JPEG transcoding (csrc/jpeg_transcode.hip): the step between ssn_jpeg_entropy and ssn_jpeg_enc_count that jpegtran does on
 * the host between its reader and its writer.  desc int32 [images][desc_ints]: ncomp, hs, vs, mcux, mcuy, first source block, first
 * destination block, blocks.
 *  layout    ints of a desc row.
 *  blocks    zero-fills status int32 [images], then src int16 [src_blocks][64] (natural order, blocks planar per image: luma raster
 *            over the padded MCU grid, Cb, Cr) -> dst int16 [dst_blocks][64] (zigzag order, blocks in scan order, dummy blocks
 *            included).  Values are copied, never changed.  A row that is inconsistent or reaches past either buffer sets status bit 4
 *            (the encoder's "unusable desc row") and writes nothing.  Both buffers 16-byte aligned. */
int ssn_jpeg_transcode_layout(int* desc_ints);
int ssn_jpeg_transcode_blocks(const short* src, long src_blocks, const int* desc, int n_images, int max_blocks, short* dst,
                              long dst_blocks, int* status, hipStream_t stream);

/* The pixels of a gray image after a round trip through a baseline JPEG file, without the file (csrc/jpeg_roundtrip.hip): bit for bit
 * Image.open(f).convert("L") of what Image.fromarray(a).save(f, "JPEG", quality=) wrote.  src and dst uint8
 * [n][h][w], contiguous; dst may be src.  quant64: DEVICE int32 [64], the luma table of the quality in natural order (1 .. 255), as
 * jpeg_encode.quant_tables builds it.  Per 8 x 8 block: level shift, the encoder's forward DCT and quantisation, multiplication by
 * the table, the decoder's inverse DCT and range limit; blocks over the right or bottom edge read the edge pixel repeated and store
 * only what is inside the image. */
int ssn_jpeg_roundtrip_gray(const unsigned char* src, unsigned char* dst, int n, int h, int w, const int* quant64, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SSN_HIP_H */
