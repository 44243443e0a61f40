/*
 * unet_hip.h -- C ABI of the MI355X (gfx950) U-Net segmentation engine.
 *
 * The reference (deadskull7/One-Stop-for-COVID-19-...) has NO native/FFI boundary of its
 * own: its hot path is Keras calls inside two Python runners.  Each entry point below
 * therefore cites the Keras call site it replaces (paths relative to
 * /root/reference/Scripts/; T1 = task1_preprocessing_plus_unet_with_comments.py,
 * T3 = task3_lung_segmentation_unet.py, which is line-for-line the same graph/recipe).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no C++/torch types cross the boundary.
 *   - every function returns int32 status: 0 = ok, <0 = error (unet_last_error(ctx)).
 *   - the CALLER owns every tensor buffer (device memory, fp32, NHWC = Keras channels_last).
 *     `ld*` arguments are the pixel stride in floats, so an op can read/write a channel
 *     slice of a wider NHWC buffer (zero-copy skip concatenation, T1:887).
 *   - all launches are asynchronous on the passed hipStream_t (`void* stream`); no hidden
 *     synchronisation, no allocation after unet_ctx_create.  State outside the caller's buffers: the ctx -- it owns two small device
 *     scratch areas (BatchNorm reduction slots; the split weight image of a ConvT launch), so launches through ONE ctx belong on one stream
 *     at a time -- and its options (unet_ctx_set_option).  The library reads NO environment variables: the kernel family is the `algo`
 *     argument of every convolution entry point / of unet_model_create, the graph-level choices are ctx options.
 *   - there is NO CPU fallback: without a gfx950 device unet_ctx_create fails.
 */
#ifndef UNET_HIP_H
#define UNET_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNET_ABI_VERSION 16

typedef struct unet_ctx unet_ctx;
typedef struct unet_model unet_model;
/* bf16 storage element (raw bit pattern; round-to-nearest-even from fp32) of the mixed-precision path */
typedef uint16_t unet_bf16;
enum { UNET_DTYPE_F32 = 0, UNET_DTYPE_BF16 = 1 };

/* status codes */
enum { UNET_OK = 0, UNET_E_ARG = -1, UNET_E_HIP = -2, UNET_E_SHAPE = -3, UNET_E_STATE = -4, UNET_E_NODEV = -5 };

/* kernel family of the convolutions (all are HIP kernels):
 *   AUTO  : fp32 conv3x3 / ConvT forward, data gradient and weight gradient as three v_mfma_f32_32x32x16_f16 products of a block-scaled two-term fp16 split
 *           (fp32-class accuracy inside the domain DESIGN.md 4g states) wherever the channel counts allow (multiples of 16 / 32), else as MFMA;
 *   MFMA  : STRICT fp32 -- v_mfma_f32_32x32x2_f32 kernels (exact fp32 multiply-add), VALU kernels for the shapes those do not take; the fallback for
 *           tensors outside the split's domain and the on-device reference of its accuracy claims;
 *   NAIVE : fp32 VALU kernels only (cross-check). */
enum { UNET_ALGO_AUTO = 0, UNET_ALGO_NAIVE = 1, UNET_ALGO_MFMA = 2 };

int32_t unet_abi_version(void);
int32_t unet_ctx_create(int32_t device_id, unet_ctx** out);
void unet_ctx_destroy(unet_ctx* ctx);
const char* unet_last_error(const unet_ctx* ctx);
/* 1 = op-level timing with hipEvents (bench.py roofline leg); adds a sync per op */
int32_t unet_ctx_set_profiling(unet_ctx* ctx, int32_t on);
/* Options of a context (defaults = the shipped path).  A model reads them when it is CREATED (unet_model_create), op-level entry points when they launch;
 * so one process can hold models / contexts of different settings side by side.
 *   RELU_BITS (1)          ReLU masks of the data gradients as one bit per element, written by the producing conv (0: the fp32 activation is re-read)
 *   BN_FOLD (2)            decoder BatchNormalization folded into the conv behind it: 0 = explicit statistics / apply passes, 1 = forward + weight gradient +
 *                          backward sums folded, 2 = also the BatchNorm backward applied in the data-gradient epilogue, 3 = as 2 and the classifier's
 *                          16-channel first block too (T2:748-751: +15 % on that step; its folded pre-activations carry more round-off -- the raw
 *                          activations have a large mean -- so at 224 x 224 x 256 about twice as many ReLU decisions differ from a float64 evaluation)
 *   ENC_BN_FUSED (1)       encoder tail backward without a statistics pass (sums from the pooled tensors + closed-form skip term, one fused apply pass)
 *   BN_CONCAT_ANALYTIC (1) decoder BatchNorm statistics: skip half from the encoder layer's sums, only the upsampled half measured
 *   BN_FUSE_STATS (1)      BatchNorm statistics accumulated by the producing conv's epilogue (unet_request_bn_stats honoured)
 *   DETERMINISTIC (0)      1 = no floating-point atomics anywhere, so reruns are bit-identical: the reductions of the stand-alone passes go through per-workgroup slots
 *                          folded in index order; the sums a kernel EPILOGUE takes (BatchNorm statistics, the fused head's loss / gradient sums, the pooled sums -- launches
 *                          with far more workgroups than slots) leave as exact integer window sums, four 64-bit words per value, whose addition is associative
 *                          (ABI v15: the same fused graph as the default mode; 1.6 % of the step, 9 % before).  Domain of an epilogue partial sum: |t| < 2^60,
 *                          bits below 2^-80 dropped; outside it (and for Inf / NaN) the folded value is NaN.  What goes into the windows is a workgroup's fp32
 *                          partial sum: of one tile in the h2 kernels; in the persistent schedule (CONV_PP) of ALL tiles of a workgroup, added per lane in fp32 --
 *                          its statistics are reproducible on a given device (the tile walk follows the CU count) but carry the rounding of that longer fp32
 *                          chain (tiles per half-workgroup x 8 additions per lane, relative to sum |y|), they are not exact sums of the stored tensor
 *   HEAD_FUSED (1)         fp32 U-Net, h2 kernels: the 1x1 sigmoid head (T1:913), the loss sums and the per-channel sums of the head's weight gradient come out of
 *                          the epilogue of the last conv3x3 (no pass over its 32-channel output in forward; backward writes dL/d(conv output) from p, the labels
 *                          and one bit per element); 0 = the separate head_fwd / head_bwd passes
 *   SKIP_RAW (1)           fp32 U-Net with BN_FOLD >= 2, ENC_BN_FUSED and BN_CONCAT_ANALYTIC: the second conv of an encoder block (T1:860) writes straight into the skip half
 *                          of its concat (T1:908) and the encoder BatchNorm's output is never stored: max-pool reads the raw tensor, the folded decoder BatchNorm is
 *                          composed with the encoder one (two affine maps in a row are one).  -1 GB of writes per step at 512 x 512 x 16.  0 = the normalised copy is stored
 *   POOL_SUMS_FUSED (1)    fp32 U-Net with ENC_BN_FUSED: the pooled-path sums of an encoder tail's BatchNorm backward come out of the epilogue of the data gradient that
 *                          produces the pooled tensor's gradient (no pass over the pooled tensors); dropout-removed elements are recognised by the -0.0f the forward stored
 *   HEAD_BWD_FUSED (1)     with HEAD_FUSED and RELU_BITS: dL/d(output of the last conv3x3) = dz_p w_c [y_pc > 0] is never written as a tensor -- unet_head_dzm leaves
 *                          {dz_p, 32 mask bits} per pixel (8 bytes instead of 128) and the last conv's data gradient and weight gradient expand that stream while they
 *                          stage it (-1.5 GB of traffic per step at 512 x 512 x 16); 0 = unet_head_dy writes the fp32 tensor
 *   CONV_PP (13; default 1) the conv3x3 forward / data-gradient launches of the shallow levels (K = 32 -> 32 channels) on the persistent two-half schedule of
 *                          kernels_conv_pp.hip: one 512-thread workgroup per CU, the layer's split weight image resident in LDS, one half's MFMAs over the other half's
 *                          loads, split and stores.  Same arithmetic as the h2 kernels (one block exponent per 8 x 32 pixel tile); taken by launches of at least four tiles per
 *                          half-workgroup (2048 tiles: 512 x 512 from batch 2 up).  0 = conv_h2_kernel everywhere; 2 = also smaller launches (tests)
 *   ENC_TAIL_DGRAD (14; default 1) fp32 U-Net with SKIP_RAW, ENC_BN_FUSED and the folded decoder BatchNorm backward: the data gradient of a decoder block's first conv is split by
 *                          output-channel range.  conv3x3_dgrad_bn_bwd:c<10-k>a writes only the upsampled half of the concat's gradient; the skip half runs where the encoder
 *                          tail's backward ran (the op keeps the name bn_pool_bwd_apply:bn<k>) and finishes pool backward + K1 y + BatchNorm backward + ReLU mask on the tile it
 *                          holds -- the skip half of the concat's gradient is never written or read (one full-resolution tensor of the level's encoder width less per level and
 *                          step; a gradient tap of bn<k> is UNET_E_STATE there).  Taken by the levels whose undivided launch runs the 8-row tiles
 *                          (the split then computes bit for bit what the two launches computed) and whose two half launches each fill the resident workgroup slots at least
 *                          twice (at 512 x 512 x 16 on 256 CUs: the 512 and 256 pixel levels); 0 = the two launches of before everywhere;
 *                          2 = every level, whatever its size (tests)
 *   WGRAD_EARLY_SPLIT (15; default 0) h2 conv3x3 weight gradient (unet_conv3x3_bwd_weights and the entry behind the head stream), 1: a step of the kernel's pixel loop scales and splits
 *                          the NEXT step's fetched rows into their two fp16 planes in the gaps of its own MFMAs, at the block exponents it holds, and confirms the exponents
 *                          behind the barrier; when a block's maximum moves one (rare) the rows are fetched again and split between the barriers as with 0.  Same MFMA order,
 *                          same scales: 1 and 0 give the same bits (tests/test_gpu_wgrad_early_split.py).  Off: on one box 1 was 0.3 - 1.8 % slower per op, the loop waits for
 *                          the rows, not for the split (profiles/wgrad_early_split_ab.txt)
 *   (options 11 / 12 of ABI v13-v14 -- WGRAD_ATOMIC, C1A_RECOMPUTE -- were same-box A/B losers and left the library in v15; DESIGN.md keeps the measurements)
 */
enum { UNET_OPT_RELU_BITS = 1, UNET_OPT_BN_FOLD = 2, UNET_OPT_ENC_BN_FUSED = 3, UNET_OPT_BN_CONCAT_ANALYTIC = 4, UNET_OPT_BN_FUSE_STATS = 5, UNET_OPT_DETERMINISTIC = 6,
       UNET_OPT_HEAD_FUSED = 7, UNET_OPT_SKIP_RAW = 8, UNET_OPT_POOL_SUMS_FUSED = 9, UNET_OPT_HEAD_BWD_FUSED = 10, UNET_OPT_CONV_PP = 13, UNET_OPT_ENC_TAIL_DGRAD = 14,
       UNET_OPT_WGRAD_EARLY_SPLIT = 15 };
int32_t unet_ctx_set_option(unet_ctx* ctx, int32_t option, int32_t value);
int32_t unet_ctx_get_option(unet_ctx* ctx, int32_t option);   /* >= 0: the value; < 0: error */

/* activations of the conv epilogue and "mask modes" of the backward epilogues (derivative of the activation -- and of the
 * dropout fused behind it -- that produced a stored tensor m):
 *   UNET_MASK_RELU 1[m>0]   UNET_MASK_ELU  m>0 ? 1 : m+1   UNET_MASK_ELU_DROP  m = dropout(elu(z)), keep mask recomputed
 *   from the counter-based RNG stream (rate, seed) of that dropout */
enum { UNET_ACT_NONE = 0, UNET_ACT_RELU = 1, UNET_ACT_ELU = 2 };
enum { UNET_MASK_NONE = 0, UNET_MASK_RELU = 1, UNET_MASK_ELU = 2, UNET_MASK_ELU_DROP = 3, UNET_MASK_RELU_BITS = 9 /* see unet_request_relu_bits */ };

/* ------------------------------------------------------------------------------------
 * Op level.  Replaces: Conv2D(C,(3,3),activation='relu',padding='same')   T1:859-911
 *   y[n,i,j,o] = act(b[o] + sum_{a,b,c} x[n,i+a-1,j+b-1,c] * w[a,b,c,o]);  w is HWIO.
 * act: 'relu' (U-Net, T1:859) or 'elu' (U-Net++, task1_unet_plus_plus.py:876); drop_rate > 0 fuses the Keras Dropout
 * layer that follows the conv (task1_unet_plus_plus.py:862, 877) into the epilogue (inverted dropout, training only).
 * w_ws: device scratch of unet_conv3x3_w_ws_floats(cin, cout) floats for the prepared (split fp16) weight image of the h2 kernels; may be
 * NULL, then only the strict fp32 kernels are used.
 * ---------------------------------------------------------------------------------- */
size_t unet_conv3x3_w_ws_floats(int32_t cin, int32_t cout);
/* which family a forward / data-gradient launch of this shape resolves to: UNET_ALGO_AUTO (the fp16-split h2 kernels), _MFMA (strict fp32 MFMA) or _NAIVE (VALU) */
int32_t unet_conv3x3_pick_algo(int32_t algo, int32_t wd, int32_t cin, int32_t cout);
/* fp32-MFMA-time equivalent of that launch's matrix work: 1 (strict / VALU), 3 * 157.3 / 2500 (h2: three fp16 MFMA products per multiply) */
double unet_conv3x3_exec_ratio(int32_t algo, int32_t h, int32_t wd, int32_t cin, int32_t cout);
/* ... and of the weight-gradient launch (unet_conv3x3_bwd_weights with the workspace it asks for) */
double unet_conv3x3_wgrad_exec_ratio(int32_t algo, int32_t h, int32_t wd, int32_t cin, int32_t cout);
/* Conv2D / Conv2DTranspose followed by a training-mode BatchNormalization (T1:860-861 `Conv2D(...)(c1)` -> `BatchNormalization()(c1)`, T1:886-888
 * `Conv2DTranspose` -> `concatenate` -> `BatchNormalization`): arms the NEXT unet_conv3x3_fwd / unet_convT2x2_fwd on this context to add the
 * per-channel (sum y, sum y^2) of the values it STORES (c channels; after activation and dropout) to the context's accumulators from its epilogue,
 * where its kernel can (the fp32 h2 kernels); the unet_bn_stats / unet_bn_stats_concat call that MUST follow on that tensor then folds them instead of reading
 * the tensor again (any other kernel ignores the request and that call does its own pass -- same results either way).  c = 0 disarms. */
int32_t unet_request_bn_stats(unet_ctx*, int32_t c);
/* The ReLU mask of a data gradient as ONE BIT per element instead of the stored fp32 activation (the backward of the T1:859-860 conv pairs reads
 * `c1 > 0` only).  unet_request_relu_bits arms the NEXT unet_conv3x3_fwd (act = UNET_ACT_RELU, no dropout) on this context to also write the sign bits
 * of what it stores into `bits` (unet_relu_bits_bytes(n, h, w, cout) bytes of device memory; layout: 64-bit words [n][y][x / 8][c / 32][4], word k of an
 * 8-pixel x 32-channel cell holds bit (x % 8) * 8 + (c % 32) / 4 for the channels with c % 4 == k); that call fails with UNET_E_SHAPE if its kernel
 * cannot (ask unet_relu_bits_supported(algo, h, w, cin, cout) first: cout % 32 == 0, w % 8 == 0, the fp32 h2 kernels).  unet_conv3x3_bwd_data then takes
 * mask_src = bits with mask_mode = UNET_MASK_RELU_BITS where unet_relu_bits_supported(algo, h, w, cout, cin) holds for ITS launch (K = cout, M = cin). */
int32_t unet_relu_bits_supported(int32_t algo, int32_t h, int32_t wd, int32_t cin, int32_t cout);
size_t unet_relu_bits_bytes(int32_t n, int32_t h, int32_t wd, int32_t c);
int32_t unet_request_relu_bits(unet_ctx*, void* bits);
/* Inference on one slice (T1:1136-1137: `model.predict` on a single 512 x 512 image) leaves the deep levels with fewer workgroups than the chip has CUs, each walking a long
 * chain of dependent loads over its contraction.  unet_allow_k_slices arms the NEXT unet_conv3x3_fwd / unet_conv3x3_bwd_data on this context (no dropout, no mask, no armed
 * statistics / sign bits, fp32 h2 kernels) to contract 2-4 slices of K side by side into context-owned slabs and add them -- with the bias and the ReLU -- in a second pass,
 * where its grid is that small (fewer than 1.5 workgroups per CU, K >= 256); any other launch ignores it.  Same result up to the order of the fp32 additions, which then
 * follows the grid size: training programs (whose data-parallel ranks must add in the order of the whole batch) never arm it, and a deterministic-mode context ignores it. */
int32_t unet_allow_k_slices(unet_ctx*);
/* Largest private segment (register-spill scratch, bytes per lane) among the h2 conv3x3 / ConvT kernels this context has launched so far: a build whose register-heavy
 * instances fell over their spill cliff shows here (and nowhere in the numerics) -- the GPU test suite holds it under a bound. */
int32_t unet_ctx_max_kernel_scratch_bytes(unet_ctx*);
int32_t unet_conv3x3_fwd(unet_ctx*, const float* x, const float* w, const float* bias, float* y,
                         int32_t n, int32_t h, int32_t wd, int32_t cin, int32_t cout,
                         int32_t act, float drop_rate, uint64_t drop_seed, int32_t algo, float* w_ws, void* stream);
/* unet_conv3x3_fwd into a channel slice of a wider NHWC buffer: y points at the slice's first channel, ldy = floats per pixel of that buffer (ldy >= cout, ldy % 4 == 0;
 * else UNET_E_ARG) -- the second conv of an encoder block writing into the skip half of its concat (T1:860 -> T1:908, SKIP_RAW).  No dropout.  Only on the fp32 h2 kernels
 * (UNET_ALGO_AUTO, cin and cout multiples of 16, w_ws given; else UNET_E_STATE).  Armed statistics / sign bits / K slices are honoured and cleared as by unet_conv3x3_fwd;
 * the unet_bn_stats call that follows an armed launch takes ldx = ldy. */
int32_t unet_conv3x3_fwd_ld(unet_ctx*, const float* x, const float* w, const float* bias, float* y, int32_t ldy,
                            int32_t n, int32_t h, int32_t wd, int32_t cin, int32_t cout, int32_t act, int32_t algo, float* w_ws, void* stream);
/* dx = conv3x3(dy, flip/transposed w) * mask_factor(mask_src): the derivative of the activation (+dropout) of the layer
 * that PRODUCED x is fused here (backward of the T1:859-860 conv pairs).  mask_rate/mask_seed: UNET_MASK_ELU_DROP only.
 * wt_ws: unet_conv3x3_w_ws_floats(cin, cout) floats of scratch for the flipped / transposed weights or their split image. */
int32_t unet_conv3x3_bwd_data(unet_ctx*, const float* dy, const float* w, const float* mask_src,
                              int32_t mask_mode, float mask_rate, uint64_t mask_seed,
                              float* dx, float* wt_ws, int32_t n, int32_t h, int32_t wd,
                              int32_t cin, int32_t cout, int32_t algo, void* stream);
/* BatchNormalization -> Conv2D(3x3) of the decoder blocks (T1:888-889, 895-896, 902-903, 909-910) WITHOUT the normalised tensor: the
 * affine z = scale[c] x + shift[c] (bnp = the float[>=2*cin] scale, shift that unet_bn_finalize_* writes) is folded into the conv --
 * weights scaled per input channel, and because Keras pads z (not x) with zeros, a bias per border class: a pixel on the first / last
 * row or column sees fewer taps of the shift (16 classes, exact).  The forward then reads the raw x.  The weight gradient runs on the raw
 * x as well and is corrected: dw = scale[c] dw_raw + shift[c] S[tap][o], S = db minus the border row / column sums of dy the tap
 * excludes (plus the corner).  Only where unet_conv3x3_bnfold_supported() says so (the h2 kernels: UNET_ALGO_AUTO, cin and cout multiples of 16; cout a
 * divisor of 256); ws: unet_conv3x3_bnfold_ws_floats floats, shared by the two calls of a step; gws: as unet_conv3x3_bwd_weights.
 * bn_bwd_sums (optional, with the kernel w and bnp = scale, shift, mean, invstd): the BatchNorm's backward sums double[2*cin] =
 * (sum dz, sum dz*xhat) as unet_bn_bwd_stats accumulates them, but WITHOUT reading dz or x -- dz is this conv's data gradient, so
 * sum_p dz_c = sum_{tap,o} w[tap][c][o] S[tap][o] and sum_p dz_c x_c = sum_{tap,o} w[tap][c][o] dw_raw[tap][c][o]. */
int32_t unet_conv3x3_bnfold_supported(int32_t algo, int32_t h, int32_t wd, int32_t cin, int32_t cout);
size_t unet_conv3x3_bnfold_ws_floats(int32_t n, int32_t cin, int32_t cout);
int32_t unet_conv3x3_bnfold_fwd(unet_ctx*, const float* x, const float* bnp, const float* w, const float* bias, float* y, int32_t n, int32_t h,
                                int32_t wd, int32_t cin, int32_t cout, int32_t act, int32_t algo, float* ws, void* stream);
int32_t unet_conv3x3_bnfold_bwd_weights(unet_ctx*, const float* x, const float* bnp, const float* dy, const float* w, float* dw, float* db,
                                        double* bn_bwd_sums, void* gws, size_t gws_bytes, float* ws, int32_t n, int32_t h, int32_t wd,
                                        int32_t cin, int32_t cout, int32_t algo, void* stream);
/* The data gradient of that conv with the BatchNorm's backward in its epilogue -- dz is never stored (what the conv3x3_dgrad_bn_bwd ops of the training programs launch in
 * fp32):  dx = f(x) (K0 dz + K1 x + K2),  dz = conv3x3(dy, flipped / transposed w),  K0 = scale, K1 = -scale invstd k2, K2 = scale (mean invstd k2 - k1) with
 * k1 = bn_bwd_sums[c] / count, k2 = bn_bwd_sums[cin + c] / count (bnp = scale, shift, mean, invstd: float[4*cin]; bn_bwd_sums = double[2*cin] as
 * unet_conv3x3_bnfold_bwd_weights leaves them; count = pixels the statistics ran over, >= 1).  f = the derivative of what produced x: mask_mode UNET_MASK_NONE (1),
 * _RELU (x > 0), _ELU, _ELU_DROP (mask_rate / mask_seed of that dropout).  x_channels = cin, or -- UNET_MASK_NONE only -- a multiple of 32 below it: channels from
 * there on do not read x and leave as K0 dz + K2 (the skip half of a concat whose consumer adds K1 x); anything else is UNET_E_ARG.  wt_ws: as unet_conv3x3_bwd_data;
 * coef: 3*cin floats of scratch.  UNET_E_SHAPE where unet_conv3x3_bnfold_supported() says no. */
int32_t unet_conv3x3_bnfold_bwd_data(unet_ctx*, const float* dy, const float* w, const float* bnp, const double* bn_bwd_sums, double count, const float* x,
                                     int32_t x_channels, int32_t mask_mode, float mask_rate, uint64_t mask_seed, float* dx, float* wt_ws, float* coef,
                                     int32_t n, int32_t h, int32_t wd, int32_t cin, int32_t cout, int32_t algo, void* stream);
/* The skip half of that data gradient with the encoder tail's backward in its epilogue (added without an ABI bump; what the bn_pool_bwd_apply ops of the training programs
 * launch where UNET_OPT_ENC_TAIL_DGRAD applies).  The conv has 2 c input channels -- the concat [upsampled | skip] -- and c output channels: dy [n,h,wd,c], w [3][3][2c][c],
 * bnp / bn_bwd_sums / count of the decoder BatchNorm as above (float[8 c], double[4 c]).  Only the output channels [c, 2 c) are computed, and instead of g = K0 dz + K2 the call
 * writes the gradient of the encoder conv output x behind BatchNorm -> max-pool 2x2 + dropout, exactly as unet_conv3x3_bnfold_bwd_data (x_channels = c) followed by
 * unet_bn_maxpool_bwd_apply (g_skip = that skip half) evaluates it, operation for operation:
 *   y = scale_e x + shift_e;  t = k1s y + g + (this pixel is the FIRST maximum of y over its 2x2 window ? dy_pooled keep : 0);
 *   dx = x > 0 ? scale_e (t - k1 - (x - mean_e) invstd_e k2) : 0,   k1 = enc_sums[j] / enc_count, k2 = enc_sums[c + j] / enc_count
 * x: the skip channels of the raw concat (pointer to channel c of pixel 0, pixel stride ldx >= c, ldx % 4 == 0); enc_bnp = scale, shift, mean, invstd of the encoder BatchNorm
 * (float[4 c]); enc_sums double[2 c] = its reduced backward sums; skip_k1 float[c] = the decoder's K1 of the skip channels (coef + 3 c of a unet_conv3x3_bnfold_bwd_data call
 * on the same sums) or NULL for k1s = 0; dy_pooled [n,h/2,wd/2,c]; rate / seed: the dropout behind the pool (keep = 0 or 1 / (1 - rate), unet_bn_apply_maxpool_dropout_fwd's
 * stream); dx [n,h,wd,c] dense.  wt_ws: unet_conv3x3_w_ws_floats(2 c, c) floats; coef: 6 c floats of scratch.  h and wd even, c a multiple of 32, and
 * unet_conv3x3_bnfold_supported(algo, h, wd, 2 c, c); else UNET_E_SHAPE. */
int32_t unet_conv3x3_bnfold_bwd_data_enc_tail(unet_ctx*, const float* dy, const float* w, const float* bnp, const double* bn_bwd_sums, double count, const float* x, int32_t ldx,
                                              const float* enc_bnp, const double* enc_sums, double enc_count, const float* skip_k1, const float* dy_pooled, float rate,
                                              uint64_t seed, float* dx, float* wt_ws, float* coef, int32_t n, int32_t h, int32_t wd, int32_t c, int32_t algo, void* stream);
/* dw[a,b,c,o] = sum x[n,i+a-1,j+b-1,c]*dy[n,i,j,o];  db[o] = sum dy.  dy already ReLU-masked.
 * ws: split-K scratch (unet_conv3x3_bwd_weights_ws_bytes). dw/db are OVERWRITTEN. */
size_t unet_conv3x3_bwd_weights_ws_bytes(int32_t n, int32_t h, int32_t wd, int32_t cin, int32_t cout);
int32_t unet_conv3x3_bwd_weights(unet_ctx*, const float* x, const float* dy, float* dw, float* db,
                                 void* ws, size_t ws_bytes, int32_t n, int32_t h, int32_t wd,
                                 int32_t cin, int32_t cout, int32_t algo, void* stream);

/* Replaces: Conv2DTranspose(C,(2,2),strides=(2,2),padding='same') + concatenate([u,c])
 * T1:886-887 (and 893-894, 900-901, 907-908).  Kernel layout [2,2,Cout,Cin] (Keras).
 *   u[n,2i+a,2j+b,o] = bias[o] + sum_c x[n,i,j,c] * w[a,b,o,c]
 * y is written with pixel stride ldy (the first Cout channels of the concat buffer). */
int32_t unet_convT2x2_fwd(unet_ctx*, const float* x, const float* w, const float* bias, float* y,
                          int32_t ldy, int32_t n, int32_t h, int32_t wd, int32_t cin, int32_t cout,
                          int32_t algo, void* stream);
int32_t unet_convT2x2_bwd_data(unet_ctx*, const float* dy, int32_t lddy, const float* w,
                               const float* relu_src, float* dx, int32_t n, int32_t h, int32_t wd,
                               int32_t cin, int32_t cout, int32_t algo, void* stream);
/* dw [2,2,Cout,Cin] and db are OVERWRITTEN; ws: split-K scratch (unet_convT2x2_bwd_weights_ws_bytes) */
size_t unet_convT2x2_bwd_weights_ws_bytes(int32_t n, int32_t h, int32_t wd, int32_t cin, int32_t cout);
int32_t unet_convT2x2_bwd_weights(unet_ctx*, const float* x, const float* dy, int32_t lddy,
                                  float* dw, float* db, void* ws, size_t ws_bytes, int32_t n,
                                  int32_t h, int32_t wd, int32_t cin, int32_t cout, int32_t algo,
                                  void* stream);

/* Replaces: BatchNormalization()  T1:861,867,873,879,888,895,902,909 (eps 1e-3, momentum .99)
 * Training forward = stats -> [optional cross-rank all-reduce of `sums`] -> finalize -> apply.
 *   sums: double[2*C] = (sum x, sum x^2), ACCUMULATED (zero it first: unet_zero).
 *   bnp : float[4*C]  = scale, shift, mean, invstd.
 *   count = elements per channel over the GLOBAL batch (n*h*w*world).
 * The statistics kernels (unet_bn_stats, unet_bn_bwd_stats, unet_maxpool2x2_dropout_bwd_bnstats) stage their atomics in a scratch the
 * CONTEXT owns: issue them on one stream at a time per context; use one context per stream otherwise. */
int32_t unet_bn_stats(unet_ctx*, const float* x, int32_t ldx, double* sums, int64_t pixels,
                      int32_t c, void* stream);
/* Statistics of the decoder's BatchNormalization over concatenate([u, c]) (T1:887-888, 894-895, 901-902, 908-909) when the skip half `c`
 * is the output of an encoder BatchNormalization of the same step: over the batch that output has mean beta and variance
 * gamma^2 var/(var + eps) exactly, so only the c_up channels of `u` (x_up, row stride ldx) are read; the c_skip pairs come from the
 * source layer's sums (src_sums = its double[2*c_skip] AFTER any cross-rank reduction, src_count = its global element count) and
 * parameters.  sums: double[2*(c_up+c_skip)] = (sums, sums of squares) of the concat, ACCUMULATED like unet_bn_stats; the analytic half is
 * scaled by `pixels` (this rank's count) so a cross-rank SUM of `sums` stays correct. */
int32_t unet_bn_stats_concat(unet_ctx*, const float* x_up, int32_t ldx, const double* src_sums, double src_count, const float* src_gamma,
                             const float* src_beta, double* sums, int64_t pixels, int32_t c_up, int32_t c_skip, void* stream);
int32_t unet_bn_finalize_train(unet_ctx*, const double* sums, double count, const float* gamma,
                               const float* beta, float* moving_mean, float* moving_var,
                               float* bnp, int32_t c, void* stream);
int32_t unet_bn_finalize_infer(unet_ctx*, const float* gamma, const float* beta,
                               const float* moving_mean, const float* moving_var, float* bnp,
                               int32_t c, void* stream);
int32_t unet_bn_apply(unet_ctx*, const float* x, int32_t ldx, const float* bnp, float* y,
                      int32_t ldy, int64_t pixels, int32_t c, void* stream);
/* backward: sums = double[2*C] (sum dy, sum dy*xhat), accumulated.  param_grads writes
 * dgamma/dbeta from the LOCAL sums (call before any cross-rank reduction of sums).
 * apply: dx = scale*(dy - sum_dy/count - xhat*sum_dyxhat/count) * mask_factor(x) (UNET_MASK_*: the derivative of what
 * produced the BN input x; UNET_MASK_ELU_DROP needs a dense x). */
int32_t unet_bn_bwd_stats(unet_ctx*, const float* dy, int32_t lddy, const float* x, int32_t ldx,
                          const float* bnp, double* sums, int64_t pixels, int32_t c, void* stream);
int32_t unet_bn_bwd_param_grads(unet_ctx*, const double* sums, float* dgamma, float* dbeta,
                                int32_t c, void* stream);
int32_t unet_bn_bwd_apply(unet_ctx*, const float* dy, int32_t lddy, const float* x, int32_t ldx,
                          const float* bnp, const double* sums, double count, int32_t mask_mode,
                          float mask_rate, uint64_t mask_seed, float* dx, int32_t lddx, int64_t pixels,
                          int32_t c, void* stream);

/* Replaces: MaxPooling2D((2,2)) + Dropout(0.25)  T1:862-863 (868-869, 874-875, 880-881).
 * rate 0 => plain pool.  Dropout keep-mask = counter-based RNG keyed by (seed, element index);
 * the backward recomputes it.  Ties in the max go to the first element in (di,dj) order.
 * bwd: dx[slice] (+)= routed gradient; accumulate=1 adds to what is already in dx (skip grad). */
int32_t unet_maxpool2x2_dropout_fwd(unet_ctx*, const float* x, int32_t ldx, float* y, int32_t n,
                                    int32_t h, int32_t wd, int32_t c, float rate, uint64_t seed,
                                    void* stream);
int32_t unet_maxpool2x2_dropout_bwd(unet_ctx*, const float* x, int32_t ldx, const float* dy,
                                    float* dx, int32_t lddx, int32_t n, int32_t h, int32_t wd,
                                    int32_t c, float rate, uint64_t seed, int32_t accumulate,
                                    void* stream);

/* Fused encoder tail BatchNormalization -> [skip] -> MaxPooling2D -> Dropout (T1:861-863): y = bn(x) into the concat slice
 * (ldy) and pooled = dropout(maxpool(y)) in one pass. */
int32_t unet_bn_apply_maxpool_dropout_fwd(unet_ctx*, const float* x, int32_t ldx, const float* bnp, float* y,
                                          int32_t ldy, float* pooled, int32_t n, int32_t h, int32_t wd,
                                          int32_t c, float rate, uint64_t seed, void* stream);
/* Fused backward of the same: dx[slice] += routed pool/dropout gradient (dx already holds the skip gradient) and
 * sums (double[2C], accumulated) += (sum d, sum d*xhat) of the finished gradient d, xhat = (y-beta)/gamma from the BN
 * output y (gamma != 0).  Replaces unet_maxpool2x2_dropout_bwd(accumulate=1) + unet_bn_bwd_stats. */
int32_t unet_maxpool2x2_dropout_bwd_bnstats(unet_ctx*, const float* y, int32_t ldy, const float* dy, float* dx,
                                            int32_t lddx, const float* gamma, const float* beta, double* sums,
                                            int32_t n, int32_t h, int32_t wd, int32_t c, float rate,
                                            uint64_t seed, void* stream);
/* The same encoder tail WITHOUT a pass for the statistics (fp32): the BatchNorm backward sums of the gradient g = g_skip + route(dy_pooled)
 * come from the pooled tensors alone -- the routed part touches only the arg-max elements, whose BatchNorm output is the pooled activation
 * itself (unet_maxpool2x2_dropout_bwd_sums: sum dy ks, sum dy ks (p/ks - beta)/gamma over 1/4 of the pixels) -- plus a closed-form term for
 * g_skip, which is the skip half of the DECODER BatchNorm's backward output: orthogonal to 1 exactly and to its own xhat up to
 * eps/(var+eps), and the decoder's xhat of a skip channel is gamma_e * invstd_d times the encoder's (unet_bn_bwd_skip_term adds
 * frac * gamma_d S2_d eps invstd_d^2 / gamma_e to sums[c + j]; the dec_* pointers at the decoder layer's skip channels, S2_d its
 * cross-rank-reduced sum dz*xhat, frac = this rank's share 1/world).  gamma == 0 is not supported (as in the fused form above).
 * unet_bn_maxpool_bwd_apply then does pool backward + skip add + BatchNorm backward + ReLU mask of the BN input x in ONE pass:
 * dx[.., c] = 1[x>0] scale (g - k1 - xhat k2); y = BN(x) is recomputed for the arg-max exactly as the forward stored it.
 * g_skip may be NULL (no skip connection: the classifier's Conv -> BN -> MaxPool tails, T2:752-754 -- then the pooled sums are the whole statistics). */
int32_t unet_maxpool2x2_dropout_bwd_sums(unet_ctx*, const float* pooled, const float* dy_pooled, const float* gamma, const float* beta, double* sums,
                                         int32_t n, int32_t h, int32_t wd, int32_t c, float rate, uint64_t seed, void* stream);
int32_t unet_bn_bwd_skip_term(unet_ctx*, double* sums, const double* dec_sum_dyxhat, const float* dec_invstd, const float* dec_gamma,
                              const float* gamma, int32_t c, double frac, void* stream);
int32_t unet_bn_maxpool_bwd_apply(unet_ctx*, const float* x, int32_t ldx, const float* bnp, const double* sums, double count, const float* g_skip,
                                  int32_t ldg, const float* dy_pooled, float* dx, int32_t lddx, int32_t n, int32_t h, int32_t wd, int32_t c,
                                  float rate, uint64_t seed, void* stream);

/* Replaces: Conv2D(1,(1,1),activation='sigmoid') T1:913 fused with the reductions of
 * bce_dice_loss / dice_coeff T1:784-799.  p = sigmoid(b + x.w).  If y_true != NULL,
 * loss_sums (double[4], accumulated) += (sum bce_elem, sum t*p, sum t, sum p). */
/* The segmentation losses of the reference's scripts (T1:784-835), chosen at compile time in Keras (`compile(loss=...)`).  All of them are functions of the
 * same four batch sums (sum l, I = sum t p, St = sum t, Sp = sum p) that the head ops accumulate, and every one has a head-logit gradient of the form
 *   dz = cb a + q (A t + B)      (a = dBCE/dz = p_clipped - t inside the clip range, 0 outside; q = p (1 - p))
 * with batch scalars cb, A, B of the global sums:
 *   UNET_LOSS_BCE_DICE  0.5 sum l / N + 0.5 (1 - D), D = (2 I + 1) / S, S = St + Sp + 1   (bce_dice_loss T1:797, the default)
 *   UNET_LOSS_BCE       sum l / N                                                         (binary_crossentropy, T1:60)
 *   UNET_LOSS_DICE      1 - D                                                             (dice_loss T1:792)
 *   UNET_LOSS_TVERSKY   1 - I / (I + alpha (Sp - I) + beta (St - I))                      (tversky_loss T1:801; T1 has alpha = beta = 0.5; both must be > 0)
 *   UNET_LOSS_WEIGHTED_BCE_DICE  0.5 sum w l / sum w + 0.5 (1 - D)                         (weighted_bce_dice_loss T1:835; dz = cb w a + ...)
 * The weighted loss takes a FIFTH sum, Sw = sum w, and weighs the first: its loss_sums are (sum w l, I, St, Sp, sum w), and its weight map w (unet_loss_weight_map)
 * goes to every head op.  The metric stays dice_coeff = D for every loss. */
enum { UNET_LOSS_BCE_DICE = 0, UNET_LOSS_BCE = 1, UNET_LOSS_DICE = 2, UNET_LOSS_TVERSKY = 3, UNET_LOSS_WEIGHTED_BCE_DICE = 4 };
/* weighted_bce_dice_loss's weight map (T1:837-845): weight[n,h,wd] = 5 exp(-5 |avg - 0.5|), avg = TF's SAME average pool of y_true[n,h,wd] over a 50 x 50 window
 * (rows r - 24 ... r + 25, columns c - 24 ... c + 25, clipped to the image; divisor = the in-image cells). */
int32_t unet_loss_weight_map(unet_ctx*, const float* y_true, float* weight, int32_t n, int32_t h, int32_t wd, void* stream);
/* unet_head_fwd / _bf16 with a weight map (NULL = unet_head_fwd): loss_sums[5] += (sum w bce, sum t p, sum t, sum p, sum w) */
int32_t unet_head_fwd_ex(unet_ctx*, const float* x, const float* w, const float* bias, float* p, const float* y_true, const float* weight_map, double* loss_sums,
                         int64_t pixels, int32_t cin, void* stream);
int32_t unet_head_fwd_bf16_ex(unet_ctx*, const unet_bf16* x, const float* w, const float* bias, float* p, const float* y_true, const float* weight_map,
                              double* loss_sums, int64_t pixels, int32_t cin, void* stream);

int32_t unet_head_fwd(unet_ctx*, const float* x, const float* w, const float* bias, float* p,
                      const float* y_true, double* loss_sums, int64_t pixels, int32_t cin,
                      void* stream);
/* loss_out float[2] = (bce_dice_loss, dice_coeff) from (globally reduced) sums; count = GLOBAL
 * number of label elements. */
int32_t unet_loss_finalize(unet_ctx*, const double* loss_sums, double count, float* loss_out,
                           void* stream);
/* backward of loss + sigmoid + 1x1 conv: dx = dz*w [*(x>0) if relu_mask: x is a ReLU conv output, T1:911], dw = sum dz*x, db = sum dz,
 * dz = dL/dp * p(1-p) with dL/dp from the GLOBAL sums.  dw/db (cin+1 floats) are ACCUMULATED. */
int32_t unet_head_bwd(unet_ctx*, const float* x, const float* w, const float* p, const float* y_true,
                      const double* loss_sums, double count, float* dx, float* dw, float* db,
                      int64_t pixels, int32_t cin, int32_t relu_mask, void* stream);
/* unet_loss_finalize / unet_head_bwd with a loss selection (UNET_LOSS_*; alpha, beta: Tversky only; weight_map: the weighted loss's, NULL for the others).
 * UNET_LOSS_BCE_DICE computes exactly what the calls without the suffix compute. */
int32_t unet_loss_finalize_ex(unet_ctx*, const double* loss_sums, double count, int32_t loss, float alpha, float beta, float* loss_out, void* stream);
int32_t unet_head_bwd_ex(unet_ctx*, const float* x, const float* w, const float* p, const float* y_true, const double* loss_sums, double count,
                         int32_t loss, float alpha, float beta, const float* weight_map, float* dx, float* dw, float* db, int64_t pixels, int32_t cin, int32_t relu_mask,
                         void* stream);

/* The data gradient of the conv BEHIND `MaxPooling2D((2, 2))` + `Dropout(0.25)` (T1:862-865: c2 = Conv2D(64)(p1) ...) together with the pooled-path sums the
 * BatchNorm in front of that pool needs for its backward (what unet_maxpool2x2_dropout_bwd_sums computes in a pass of its own):
 *   dx = conv3x3(dy, flipped w) [n,h,w,cin]  (= the gradient of the pooled tensor);  sums[2 cin] += (sum dx ks, sum dx ks (p (1 - rate) - beta) / gamma)
 * with p = `pooled`, the OUTPUT of unet_bn_apply_maxpool_dropout_fwd at the same rate: that kernel stores a dropout-removed element as -0.0f (a kept zero as
 * +0.0f), which is how ks = 1 / (1 - rate) | 0 is read back without replaying the random stream.  fp32 UNET_ALGO_AUTO kernels, cin % 32 == 0, not in
 * deterministic mode (unet_conv3x3_bwd_data_pool_sums_supported).  wt_ws as for unet_conv3x3_bwd_data. */
int32_t unet_conv3x3_bwd_data_pool_sums_supported(unet_ctx*, int32_t algo, int32_t wd, int32_t cin, int32_t cout);
int32_t unet_conv3x3_bwd_data_pool_sums(unet_ctx*, const float* dy, const float* w, const float* pooled, const float* gamma, const float* beta, float rate,
                                        float* dx, double* sums, float* wt_ws, int32_t n, int32_t h, int32_t wd, int32_t cin, int32_t cout, void* stream);

/* Replaces: `c9 = Conv2D(32, (3, 3), relu)(c9)` + `outputs = Conv2D(1, (1, 1), activation='sigmoid')(c9)` T1:911-913 and the loss sums of
 * bce_dice_loss T1:784-799 in ONE launch (fp32, UNET_ALGO_AUTO kernels, 32 output channels, W % 8 == 0, not in deterministic mode:
 * unet_conv3x3_head_supported): y = relu(conv3x3(x) + bias) [n,h,w,32], p = sigmoid(y . w_head + b_head) [n,h,w]; with y_true
 *   loss_sums[4] += (sum bce, sum t p, sum t, sum p)   -- as unet_head_fwd
 *   head_sums[99] += per channel c: sum a y_c | sum t q y_c | sum q y_c  (a = dBCE/dz = p_clipped - t inside the clip range, q = p (1 - p)), then sum a, sum t q, sum q
 * The head's weight gradient is a combination of head_sums once the batch-global Dice sums are known (unet_head_dy), so the backward needs no pass
 * over y.  ReLU sign bits of y can be requested as for unet_conv3x3_fwd (unet_request_relu_bits).  w_ws: unet_conv3x3_w_ws_floats(cin, 32) floats.
 * y may be NULL: the 32-channel tensor is then not stored (a backward through unet_head_dzm reads p, the sums and the sign bits only; inference reads p). */
int32_t unet_conv3x3_head_supported(unet_ctx*, int32_t algo, int32_t w, int32_t cin, int32_t cout);
int32_t unet_conv3x3_head_fwd(unet_ctx*, const float* x, const float* w, const float* bias, float* y, const float* w_head, const float* b_head, float* p,
                              const float* y_true, double* loss_sums, double* head_sums, int32_t n, int32_t h, int32_t wd, int32_t cin, float* w_ws, void* stream);
/* backward of that head: dy[n,h,w,32] = dz w_head [y > 0] (mask from relu_bits, or from y when relu_bits is NULL), dz as in unet_head_bwd from the
 * GLOBAL loss sums; dw_head[32] / db_head[1] += the combination of head_sums. */
int32_t unet_head_dy(unet_ctx*, const float* p, const float* y_true, const double* loss_sums, double count, const double* head_sums, const float* w_head,
                     const void* relu_bits, const float* y, float* dy, float* dw_head, float* db_head, int32_t n, int32_t h, int32_t wd, void* stream);
/* The same backward without the fp32 tensor dy: it has ONE fp32 degree of freedom and 32 mask bits per pixel, so unet_head_dzm writes the stream
 * dzm[n,h,w] = {float dz, uint32 mask (bit c = y_c > 0)} (8 bytes per pixel instead of 128; relu_bits required; dw_head / db_head += as unet_head_dy) and the two
 * gradients of the conv in front of the head (`Conv2D(32, (3, 3), relu)`, T1:911) expand it while they stage it:
 *   unet_conv3x3_bwd_data_dzm     dx[n,h,w,cin] = conv3x3_bwd_data(dy, w) with w_head folded into the weight image; relu_bits_in (or NULL) = the ReLU bits of the conv's INPUT
 *                                 (unet_request_relu_bits on the launch that produced it); wt_ws as for unet_conv3x3_bwd_data
 *   unet_conv3x3_bwd_weights_dzm  dw[3][3][cin][32], db[32] = conv3x3_bwd_weights(x, dy) (overwritten), the head's weights applied to the finished columns; ws as for
 *                                 unet_conv3x3_bwd_weights(cin, 32)
 * fp32 UNET_ALGO_AUTO kernels, cin = 32, W % 8 == 0 (unet_head_bwd_stream_supported). */
int32_t unet_head_bwd_stream_supported(unet_ctx*, int32_t algo, int32_t wd, int32_t cin);
int32_t unet_head_dzm(unet_ctx*, const float* p, const float* y_true, const double* loss_sums, double count, const double* head_sums, const void* relu_bits, void* dzm,
                      float* dw_head, float* db_head, int32_t n, int32_t h, int32_t wd, void* stream);
/* unet_conv3x3_head_fwd with a weight map (NULL = unet_conv3x3_head_fwd): loss_sums[5] as unet_head_fwd_ex, and the first per-channel head sum is sum w a y_c */
int32_t unet_conv3x3_head_fwd_ex(unet_ctx*, const float* x, const float* w, const float* bias, float* y, const float* w_head, const float* b_head, float* p,
                                 const float* y_true, const float* weight_map, double* loss_sums, double* head_sums, int32_t n, int32_t h, int32_t wd, int32_t cin,
                                 float* w_ws, void* stream);
/* unet_head_dy / unet_head_dzm with a loss selection (as unet_head_bwd_ex) */
int32_t unet_head_dy_ex(unet_ctx*, const float* p, const float* y_true, const double* loss_sums, double count, const double* head_sums, int32_t loss, float alpha,
                        float beta, const float* weight_map, const float* w_head, const void* relu_bits, const float* y, float* dy, float* dw_head, float* db_head, int32_t n, int32_t h,
                        int32_t wd, void* stream);
int32_t unet_head_dzm_ex(unet_ctx*, const float* p, const float* y_true, const double* loss_sums, double count, const double* head_sums, int32_t loss, float alpha,
                         float beta, const float* weight_map, const void* relu_bits, void* dzm, float* dw_head, float* db_head, int32_t n, int32_t h, int32_t wd, void* stream);
int32_t unet_conv3x3_bwd_data_dzm(unet_ctx*, const void* dzm, const float* w, const float* w_head, const void* relu_bits_in, float* dx, float* wt_ws, int32_t n, int32_t h,
                                  int32_t wd, int32_t cin, void* stream);
int32_t unet_conv3x3_bwd_weights_dzm(unet_ctx*, const float* x, const void* dzm, const float* w_head, float* dw, float* db, void* ws, size_t ws_bytes, int32_t n, int32_t h,
                                     int32_t wd, int32_t cin, void* stream);

/* Replaces: Adam(lr=0.0005) step of model.fit T1:1053,1059 -- Keras-2.3 form:
 *   m=b1 m+(1-b1)g; v=b2 v+(1-b2)g^2; p -= lr_t*m/(sqrt(v)+eps), lr_t=lr*sqrt(1-b2^t)/(1-b1^t)
 * (lr_t computed by the caller).  One launch over the flat parameter buffer. */
int32_t unet_adam_keras(unet_ctx*, float* p, const float* g, float* m, float* v, int64_t count,
                        float lr_t, float b1, float b2, float eps, float grad_scale, void* stream);

/* Replaces: sm.metrics.IOUScore/FScore/Precision/Recall(threshold=t) evaluate sweeps
 * T1:1205-1211, 1259-1265, 1313-1319: out double[T*3] += (sum gt*pr, sum pr, sum gt), pr=(p>t). */
int32_t unet_seg_metrics_sweep(unet_ctx*, const float* p, const float* gt, const float* thresholds,
                               int32_t nthr, double* out, int64_t count, void* stream);

/* Replaces: the batch slicing of model.fit (T1:1059-1061; Keras takes `x[batch_ids]` of a shuffled index array per step) for a dataset that was
 * uploaded ONCE: dst[i] = src[idx[i]], whole samples of sample_floats floats (a multiple of 4); idx = int64 sample numbers on the device. */
int32_t unet_gather_samples(unet_ctx*, const float* src, const int64_t* idx, float* dst, int64_t n,
                            int64_t sample_floats, void* stream);

/* Replaces: the reference's augmentation `seq(images=..., segmentation_maps=...)` (imgaug Fliplr / Flipud / Affine, T1:547-583) for a training batch, on the
 * device.  dst_img[i] = src_img[idx[i]] warped through mats[6 i .. 6 i + 5] with bilinear taps (NHWC, c channels), dst_mask[i] = src_mask[idx[i]] warped with
 * nearest-neighbour taps (floor(s + 0.5); one channel); both read 0 outside the source.  mats[i] = the INVERSE map of sample i, output pixel -> source pixel:
 * (x, y) -> (m0 x + m1 y + m2, m3 x + m4 y + m5), pixel centres at integers (augment.py states the policy that builds it).  idx = int64 sample numbers on the
 * device, or null for i -> i; src_mask / dst_mask both null: images only.  Any h, w; 64-bit sample offsets.  Bad arguments: UNET_E_ARG. */
int32_t unet_augment_samples(unet_ctx*, const float* src_img, const float* src_mask, const int64_t* idx, const float* mats, float* dst_img, float* dst_mask,
                             int64_t n, int32_t h, int32_t w, int32_t c, void* stream);

/* Replaces: the reference's feature-tap clustering (T1:1386-1496): sklearn PCA(n_components=1000) + KMeans(n_clusters=2) over the flattened conv2d_9
 * activations, on the device (cluster.py builds PCA / KMeans on these entries).  Every input is fp32, row-major, with a leading dimension in elements;
 * every offset is 64-bit (matrices beyond 2^31 bytes are fine); every reduction runs in a fixed order (no floating-point atomics): reruns are bit-identical.
 * Bad arguments: UNET_E_ARG. */
enum { UNET_FEAT_OUT_F32 = 0, UNET_FEAT_OUT_F64 = 1 };
/* mu[j] = (1/n) sum_i x[i * ldx + j], j < d, accumulated in fp64 in row order.  mu: d doubles. */
int32_t unet_feat_col_mean(unet_ctx*, const float* x, int64_t ldx, int64_t n, int64_t d, double* mu, void* stream);
/* Bytes of workspace unet_feat_gemm_nt needs for this shape (0: none). */
size_t unet_feat_gemm_nt_workspace(int64_t m, int64_t p, int64_t d, int32_t sym);
/* Centred NT product C[m x p] = (A - 1 mu_a^T)(B - 1 mu_b^T)^T: C[i][j] = sum_{t<d} (a[i * lda + t] - mu_a[t]) (b[j * ldb + t] - mu_b[t]).  mu_a / mu_b:
 * d doubles each, or null for no mean; each is rounded to fp32 and subtracted as the operand is staged.  v_mfma_f32_32x32x2_f32 products, fp32 within a
 * K block of 32, fp64 across blocks and across the K slabs of a split (added in slab order).  sym = 1 (the Gram matrix: a == b, lda == ldb,
 * mu_a == mu_b, m == p): only the upper-triangle tiles are computed and mirrored, C is exactly symmetric.  c: fp32 or fp64 (c_dtype UNET_FEAT_OUT_*),
 * leading dimension ldc.  ws: device scratch of unet_feat_gemm_nt_workspace(m, p, d, sym) bytes. */
int32_t unet_feat_gemm_nt(unet_ctx*, const float* a, int64_t lda, const double* mu_a, const float* b, int64_t ldb, const double* mu_b, int64_t m,
                          int64_t p, int64_t d, int32_t sym, void* c, int64_t ldc, int32_t c_dtype, void* ws, size_t ws_bytes, void* stream);
/* Bytes of workspace unet_feat_gemm_tn needs for this shape (0: none). */
size_t unet_feat_gemm_tn_workspace(int64_t k, int64_t d, int64_t n);
/* Combine (TN) product out[k x d] = W^T (X - 1 mu^T): out[r][j] = sum_{i<n} w[i * ldw + r] (x[i * ldx + j] - mu[j]).  W: n x k, X: n x d, mu: d doubles
 * or null.  The tile core of unet_feat_gemm_nt with the reduction over the sample axis.  out: fp32 or fp64 (out_dtype), leading dimension ldo; ws: device
 * scratch of unet_feat_gemm_tn_workspace(k, d, n) bytes. */
int32_t unet_feat_gemm_tn(unet_ctx*, const float* w, int64_t ldw, const float* x, int64_t ldx, const double* mu, int64_t n, int64_t k, int64_t d,
                          void* out, int64_t ldo, int32_t out_dtype, void* ws, size_t ws_bytes, void* stream);
/* One Lloyd step (and KMeans.predict): points P (n x p fp32, leading dimension ldp), centres (k x p fp64, dense).  labels[i] = argmin_c ||P_i - centre_c||^2
 * (fp64 distances from direct differences; the lower index wins a tie), dist[i] = that squared distance, sums[c][j] = sum over the points of cluster c
 * of P[i][j] in fp64 (point order; k x p dense), counts[c] = their number, *inertia = sum_i dist[i].  One launch. */
int32_t unet_kmeans_step(unet_ctx*, const float* pts, int64_t ldp, int64_t n, int64_t p, const double* centres, int32_t k, int32_t* labels,
                         double* dist, double* sums, int64_t* counts, double* inertia, void* stream);
/* Routing (routed.py: a new slice goes to its cluster's expert, the plan the reference states above T1:1386): the PCA projection of a batch of taps and its
 * nearest centre, fused.  tap: the engine's NHWC view [n][h][w] with pixel stride ld >= c (fp32, or bf16 widened to fp32 when tap_bf16), read in place.
 * comps_hwc: k x d fp32 (d = h * w * c), the PCA components permuted into tap order (h, w, c); mu_hwc: d fp32 (the PCA mean rounded to fp32, subtracted
 * term by term as operands are staged), or null.  proj[i][r] = sum_t (x_i[t] - mu[t]) comps[r][t] with the precision of unet_feat_gemm_nt (fp32 within K
 * blocks of 32, fp64 across blocks and across K slabs, added in slab order), rounded to fp32 (n x k, or null: not stored).  labels[i] / dist[i] as
 * unet_kmeans_step against centres (nc x k fp64, dense): fp64 squared distances by direct differences from the fp32 projections, the lowest index wins a
 * tie.  The reduction order depends on (d, k) only -- never on n or on a row's position -- so a row's outputs are bit-identical alone or in any batch, and
 * reruns are bit-identical (no floating-point atomics).  64-bit addressing.  Two launches.  ws: device scratch of unet_cluster_route_workspace(n, d, k)
 * bytes.  Bad arguments (nc outside 1..16, k < 1, ld < c, a short workspace): UNET_E_ARG. */
size_t unet_cluster_route_workspace(int64_t n, int64_t d, int32_t k);
int32_t unet_cluster_route(unet_ctx*, const void* tap, int32_t tap_bf16, int64_t n, int32_t h, int32_t w, int32_t c, int64_t ld,
                           const float* comps_hwc, const float* mu_hwc, int32_t k, const double* centres, int32_t nc,
                           float* proj, int32_t* labels, double* dist, void* ws, size_t ws_bytes, void* stream);

int32_t unet_zero(unet_ctx*, void* ptr, size_t bytes, void* stream);
/* concatenate([...]) of a tensor that feeds SEVERAL concats (U-Net++ nested skips, task1_unet_plus_plus.py:891-923):
 * copy a dense/sliced tensor into a channel slice of a concat buffer; and the backward: dst (+)= sum of <= 4 gradient slices */
int32_t unet_copy_slice(unet_ctx*, const float* src, int32_t lds, float* dst, int32_t ldd, int64_t pixels, int32_t c, void* stream);
int32_t unet_accum_slices(unet_ctx*, const float* const* srcs, const int32_t* lds, int32_t nsrc, float* dst, int32_t ldd,
                          int64_t pixels, int32_t c, int32_t accumulate, void* stream);

/* ---- bf16-storage variants of the ops above (ABI v5) ----------------------------------------------------------------
 * Mixed precision of the same graph: activations and activation gradients are unet_bf16 in HBM (half the traffic), parameters,
 * parameter gradients, BN sums (fp64), the head's probabilities / targets and all arithmetic stay fp32; convolutions run on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Same argument meaning as the fp32 functions; `ld*` in ELEMENTS.
 * Channel counts: conv3x3 forward cin % 16 == 0 (or the cin == 1 `first` entry points, whose image stays fp32) and cout % 16 == 0,
 * so a layer that is also differentiated needs both multiples of 16; convT cin, cout % 32 == 0; other shapes return UNET_E_SHAPE.  w_ws: device scratch of unet_conv3x3_w_ws_floats(cin, cout)
 * floats (re-laid-out bf16 weights).  BASELINE.json configs[3], configs[4] name bf16. */
int32_t unet_cast_f32_to_bf16(unet_ctx*, const float* src, unet_bf16* dst, int64_t count, void* stream);   /* count % 4 == 0 */
int32_t unet_cast_bf16_to_f32(unet_ctx*, const unet_bf16* src, float* dst, int64_t count, void* stream);
int32_t unet_conv3x3_fwd_bf16(unet_ctx*, const unet_bf16* x, const float* w, const float* bias, unet_bf16* y, int32_t n, int32_t h, int32_t wd,
                              int32_t cin, int32_t cout, int32_t act, float drop_rate, uint64_t drop_seed, void* w_ws, void* stream);
int32_t unet_conv3x3_first_fwd_bf16(unet_ctx*, const float* x, const float* w, const float* bias, unet_bf16* y, int32_t n, int32_t h,
                                    int32_t wd, int32_t cout, int32_t act, float drop_rate, uint64_t drop_seed, void* stream);
int32_t unet_conv3x3_bwd_data_bf16(unet_ctx*, const unet_bf16* dy, const float* w, const unet_bf16* mask_src, int32_t mask_mode, float mask_rate,
                                   uint64_t mask_seed, unet_bf16* dx, void* w_ws, int32_t n, int32_t h, int32_t wd, int32_t cin, int32_t cout,
                                   void* stream);
size_t unet_conv3x3_bwd_weights_ws_bytes_bf16(int32_t n, int32_t h, int32_t wd, int32_t cin, int32_t cout);
int32_t unet_conv3x3_bwd_weights_bf16(unet_ctx*, const unet_bf16* x, const unet_bf16* dy, float* dw, float* db, void* ws, size_t ws_bytes,
                                      int32_t n, int32_t h, int32_t wd, int32_t cin, int32_t cout, void* stream);
int32_t unet_conv3x3_first_bwd_weights_bf16(unet_ctx*, const float* x, const unet_bf16* dy, float* dw, float* db, void* ws, size_t ws_bytes,
                                            int32_t n, int32_t h, int32_t wd, int32_t cout, void* stream);
int32_t unet_convT2x2_fwd_bf16(unet_ctx*, const unet_bf16* x, const float* w, const float* bias, unet_bf16* y, int32_t ldy, int32_t n, int32_t h,
                               int32_t wd, int32_t cin, int32_t cout, void* w_ws, void* stream);
int32_t unet_convT2x2_bwd_data_bf16(unet_ctx*, const unet_bf16* dy, int32_t lddy, const float* w, const unet_bf16* relu_src, unet_bf16* dx,
                                    int32_t n, int32_t h, int32_t wd, int32_t cin, int32_t cout, void* w_ws, void* stream);
size_t unet_convT2x2_bwd_weights_ws_bytes_bf16(int32_t n, int32_t h, int32_t wd, int32_t cin, int32_t cout);
int32_t unet_convT2x2_bwd_weights_bf16(unet_ctx*, const unet_bf16* x, const unet_bf16* dy, int32_t lddy, float* dw, float* db, void* ws,
                                       size_t ws_bytes, int32_t n, int32_t h, int32_t wd, int32_t cin, int32_t cout, void* stream);
int32_t unet_bn_stats_bf16(unet_ctx*, const unet_bf16* x, int32_t ldx, double* sums, int64_t pixels, int32_t c, void* stream);
int32_t unet_bn_stats_concat_bf16(unet_ctx*, const unet_bf16* x_up, int32_t ldx, const double* src_sums, double src_count, const float* src_gamma,
                                  const float* src_beta, double* sums, int64_t pixels, int32_t c_up, int32_t c_skip, void* stream);
int32_t unet_bn_apply_bf16(unet_ctx*, const unet_bf16* x, int32_t ldx, const float* bnp, unet_bf16* y, int32_t ldy, int64_t pixels, int32_t c,
                           void* stream);
int32_t unet_bn_bwd_stats_bf16(unet_ctx*, const unet_bf16* dy, int32_t lddy, const unet_bf16* x, int32_t ldx, const float* bnp, double* sums,
                               int64_t pixels, int32_t c, void* stream);
int32_t unet_bn_bwd_apply_bf16(unet_ctx*, const unet_bf16* dy, int32_t lddy, const unet_bf16* x, int32_t ldx, const float* bnp, const double* sums,
                               double count, int32_t mask_mode, float mask_rate, uint64_t mask_seed, unet_bf16* dx, int32_t lddx,
                               int64_t pixels, int32_t c, void* stream);
int32_t unet_maxpool2x2_dropout_fwd_bf16(unet_ctx*, const unet_bf16* x, int32_t ldx, unet_bf16* y, int32_t n, int32_t h, int32_t wd, int32_t c,
                                         float rate, uint64_t seed, void* stream);
int32_t unet_maxpool2x2_dropout_bwd_bf16(unet_ctx*, const unet_bf16* x, int32_t ldx, const unet_bf16* dy, unet_bf16* dx, int32_t lddx, int32_t n,
                                         int32_t h, int32_t wd, int32_t c, float rate, uint64_t seed, int32_t accumulate, void* stream);
int32_t unet_bn_apply_maxpool_dropout_fwd_bf16(unet_ctx*, const unet_bf16* x, int32_t ldx, const float* bnp, unet_bf16* y, int32_t ldy,
                                               unet_bf16* pooled, int32_t n, int32_t h, int32_t wd, int32_t c, float rate, uint64_t seed,
                                               void* stream);
int32_t unet_maxpool2x2_dropout_bwd_sums_bf16(unet_ctx*, const unet_bf16* pooled, const unet_bf16* dy_pooled, const float* gamma, const float* beta,
                                              double* sums, int32_t n, int32_t h, int32_t wd, int32_t c, float rate, uint64_t seed, void* stream);
int32_t unet_bn_maxpool_bwd_apply_bf16(unet_ctx*, const unet_bf16* x, int32_t ldx, const float* bnp, const double* sums, double count,
                                       const unet_bf16* g_skip, int32_t ldg, const unet_bf16* dy_pooled, unet_bf16* dx, int32_t lddx, int32_t n,
                                       int32_t h, int32_t wd, int32_t c, float rate, uint64_t seed, void* stream);
int32_t unet_maxpool2x2_dropout_bwd_bnstats_bf16(unet_ctx*, const unet_bf16* y, int32_t ldy, const unet_bf16* dy, unet_bf16* dx, int32_t lddx,
                                                 const float* gamma, const float* beta, double* sums, int32_t n, int32_t h, int32_t wd,
                                                 int32_t c, float rate, uint64_t seed, void* stream);
int32_t unet_head_fwd_bf16(unet_ctx*, const unet_bf16* x, const float* w, const float* bias, float* p, const float* y_true, double* loss_sums,
                           int64_t pixels, int32_t cin, void* stream);
int32_t unet_head_bwd_bf16(unet_ctx*, const unet_bf16* x, const float* w, const float* p, const float* y_true, const double* loss_sums,
                           double count, unet_bf16* dx, float* dw, float* db, int64_t pixels, int32_t cin, int32_t relu_mask, void* stream);
int32_t unet_head_bwd_bf16_ex(unet_ctx*, const unet_bf16* x, const float* w, const float* p, const float* y_true, const double* loss_sums, double count,
                              int32_t loss, float alpha, float beta, const float* weight_map, unet_bf16* dx, float* dw, float* db, int64_t pixels, int32_t cin,
                              int32_t relu_mask, void* stream);
/* dense tail: the flattened activations x (and their gradient dx) are bf16, the 32 hidden units, dy and the weights stay fp32 */
int32_t unet_dense_fwd_bf16(unet_ctx*, const unet_bf16* x, const float* w, const float* bias, float* y, int32_t batch, int32_t k, int32_t n, int32_t act,
                            float drop_rate, uint64_t drop_seed, void* ws, size_t ws_bytes, void* stream);
int32_t unet_dense_bwd_bf16(unet_ctx*, const unet_bf16* x, const float* w, const float* dy, unet_bf16* dx, float* dw, int32_t batch, int32_t k, int32_t n,
                            void* stream);
int32_t unet_copy_slice_bf16(unet_ctx*, const unet_bf16* src, int32_t lds, unet_bf16* dst, int32_t ldd, int64_t pixels, int32_t c, void* stream);
int32_t unet_accum_slices_bf16(unet_ctx*, const unet_bf16* const* srcs, const int32_t* lds, int32_t nsrc, unet_bf16* dst, int32_t ldd,
                               int64_t pixels, int32_t c, int32_t accumulate, void* stream);

/* ---- dense tail of the slice classifier (task2_covid19_classifcation.py:770-776, `T2`) ------------------------------
 * Replaces: Flatten -> Dense(32, relu) -> Dropout(0.4) T2:772-775.  y[b,:] = dropout(act(x[b,:] W + bias)); x [batch,k] row-major
 * (the NHWC pooled tensor IS Keras' channels_last flatten order), W [k,n] (Keras Dense kernel), n a power of two in 4..32,
 * k %% 4 == 0.  Split-K partials in `ws` (unet_dense_ws_bytes), fixed-order reduction -> deterministic. */
size_t unet_dense_ws_bytes(int32_t batch, int32_t k, int32_t n);
int32_t unet_dense_fwd(unet_ctx*, const float* x, const float* w, const float* bias, float* y, int32_t batch, int32_t k, int32_t n,
                       int32_t act, float drop_rate, uint64_t drop_seed, void* ws, size_t ws_bytes, void* stream);
/* dx[b,:] = dy[b,:] W^T (dx may be NULL), dw = x^T dy.  dy must already carry the derivative of the activation/dropout
 * (unet_cls_head_bwd writes it that way). */
int32_t unet_dense_bwd(unet_ctx*, const float* x, const float* w, const float* dy, float* dx, float* dw, int32_t batch, int32_t k,
                       int32_t n, void* stream);
/* Replaces: Dense(1, sigmoid) T2:776 fused with loss='binary_crossentropy' (T2:829, optional class weights T2:801-803, 835) and the
 * sums of the f1 metric T2:688-703.  p[b] = sigmoid(h[b,:].w + bias).  If y_true != NULL, sums (double[4], accumulated) +=
 * (sum cw(t)*bce, sum round(t*p), sum round(t), sum round(p)); round = to nearest, ties to even; bce clips p to [1e-7, 1 - 1e-7] (fp32).
 * One workgroup; the forward takes any n that is a multiple of 4 (n >= 4). */
int32_t unet_cls_head_fwd(unet_ctx*, const float* h, const float* w, const float* bias, float* p, const float* y_true, float class_w0,
                          float class_w1, double* sums, int32_t batch, int32_t n, void* stream);
/* out float[2] = (loss = sums[0]/count, f1) from (globally reduced) sums; count = GLOBAL batch size */
int32_t unet_cls_loss_finalize(unet_ctx*, const double* sums, double count, float* out, void* stream);
/* backward of loss + sigmoid + Dense(n->1) + the Dropout/ReLU of the hidden layer h = dropout(relu(a)):
 * dw[n], db[1]; dh[batch,n] = dL/da (ready for unet_dense_bwd); dbias_prev[n] = sum_b dh[b,:] (bias gradient of the hidden Dense).
 * dz_b = cw(t_b) (p_b - t_b) / count where p_b lies inside the clip range of the loss, exactly 0 outside it.  Unlike the forward, the backward needs n to be a
 * power of two in 4..32 (as unet_dense_fwd / _bwd); any other n: UNET_E_ARG, nothing is launched. */
int32_t unet_cls_head_bwd(unet_ctx*, const float* h, const float* w, const float* p, const float* y_true, float class_w0, float class_w1,
                          double count, float drop_rate, float* dh, float* dw, float* db, float* dbias_prev, int32_t batch, int32_t n,
                          void* stream);

/* ---- image steps in front of the path: byte / integer work, bit-exact against oracle/preprocess_oracle.py ----
 * Replaces: `img = (img - xmin)/(xmax - xmin)` T1:336-337 + `np.uint8(test_img*255)` T1:165-166 (float64 arithmetic, truncation);
 *           `cv2.createCLAHE(clipLimit=3.0, tileGridSize=(8,8)).apply(img)` T1:168-169 (OpenCV clahe.cpp restated; cv2 is not in
 *           this image: parity unpinned); `cts/255` T1:520.  Images are dense [n][h][w] (single channel).
 * Min-max: an image that holds a NaN comes out all 0, as numpy's propagating min / max make it (so does a constant image: 0 / 0); an infinity zeroes the image
 * by the arithmetic alone (x / inf = 0, inf / inf = NaN -> 0).
 * Refusals, nothing launched: a null pointer, n / pixels / count / h / w / tiles < 1, clip_limit < 0, ws_bytes below the _ws_bytes function: UNET_E_ARG; CLAHE on an
 * image whose reflect-101 padding (`tiles - size % tiles` on both axes as soon as one does not divide) reaches its size: UNET_E_SHAPE. */
size_t unet_pre_minmax_ws_bytes(int32_t n);
int32_t unet_pre_minmax_to_u8(unet_ctx*, const float* img, uint8_t* out, int32_t n, int64_t pixels_per_image, void* ws, size_t ws_bytes, void* stream);
int32_t unet_pre_unit_to_u8(unet_ctx*, const float* img, uint8_t* out, int64_t count, void* stream);
int32_t unet_pre_u8_to_unit(unet_ctx*, const uint8_t* src, float* dst, int64_t count, void* stream);
size_t unet_pre_clahe_ws_bytes(int32_t n, int32_t tiles_x, int32_t tiles_y);
int32_t unet_pre_clahe_u8(unet_ctx*, const uint8_t* src, uint8_t* dst, int32_t n, int32_t h, int32_t w, float clip_limit, int32_t tiles_x,
                          int32_t tiles_y, void* ws, size_t ws_bytes, void* stream);
/* cv2.resize on uint8 crops (OpenCV resize.cpp, 8-bit path, restated: parity unpinned).  Replaces
 *   `cv2.resize(img[y:y+h, x:x+w], dsize=(125,250), interpolation=cv2.INTER_AREA)`  T1:235-238, 354-357, 364-367  (interp = 3)
 *   `cv2.resize(cts[i], dsize=(new_dim,new_dim), interpolation=cv2.INTER_LINEAR)`    T1:486-488                     (interp = 1)
 * src: dense [n][sh][sw]; rects: HOST array [n][4] = (x, y, w, h) per image in cv2.boundingRect order, or NULL for the whole image;
 * image i is written to the dh x dw window at column dst_x0 of dst[i] (rows of dst_ld bytes), so the two lung crops of a slice
 * land side by side without a concatenate (T1:358).  Interpolation values are cv2's (INTER_LINEAR = 1, INTER_AREA = 3).
 * Refusals, nothing launched: a null src / dst, a size < 1, dst_x0 < 0, dst_ld < dst_x0 + dw, another interpolation: UNET_E_ARG; dh dw >= 2^31, or a rectangle that is
 * empty or leaves the image: UNET_E_SHAPE. */
enum { UNET_RESIZE_LINEAR = 1, UNET_RESIZE_AREA = 3 };
int32_t unet_pre_resize_u8(unet_ctx*, const uint8_t* src, int32_t n, int32_t sh, int32_t sw, const int32_t* rects, uint8_t* dst, int32_t dh,
                           int32_t dw, int32_t dst_ld, int32_t dst_x0, int32_t interp, void* stream);
/* The contour search of `cropper` (T1:219-233, T3:221-235) on the HOST: `cv2.findContours(img, cv2.RETR_TREE, cv2.CHAIN_APPROX_SIMPLE)`, then
 * `cv2.contourArea(c)` and `cv2.boundingRect(c)` of every contour, for n uint8 slices (non-zero = foreground) in HOST memory [n][h][w].  Border following
 * (Suzuki-Abe, what OpenCV implements; restated: parity unpinned) is a serial walk, so it runs on CPU threads (`threads` <= 0: all cores, one slice per
 * thread at a time).  Per slice i: counts[i] = number of contours; the first min(counts[i], max_contours) areas / rects (x, y, w, h) are written in cv2's
 * output order (hierarchy pre-order, siblings newest first).  The caller does the reference's `np.argsort(areas)` and picks the two largest.
 * ctx may be NULL (no device is touched). */
int32_t unet_pre_contours_u8(unet_ctx*, const uint8_t* host_imgs, int32_t n, int32_t h, int32_t w, int32_t max_contours, double* areas, int32_t* rects,
                             int32_t* counts, int32_t threads);

/* ---- a CT volume on the device: raw NIfTI voxels -> slice batch -> mask volume (csrc/kernels_volume.hip; bit-exact against tests/volume_oracle.py) ----
 * Replaces the first half of read_nii / read_nii_demo (T1:285-297, 317-337; the same text T3:284-300): `ct_scan.get_fdata()` (float64; `scaled` != 0:
 * (float64(v) * slope) + inter, two rounded operations -- the caller applies nibabel's rules for a zero / non-finite slope and a non-finite inter),
 * `np.rot90`, `array[:, :, z0:z1]`, `cv2.resize(slice, (S, S), INTER_AREA)` on the FLOAT64 slice (OpenCV resize.cpp, 64-bit float path, restated: parity
 * unpinned) and the per-slice min-max.  vox: the whole volume on the device, Fortran order [X, Y, Z], `dtype` a NIfTI-1 datatype code
 * (2 uint8, 256 int8, 4 int16, 512 uint16, 8 int32, 768 uint32, 16 float32, 64 float64), native byte order.  Outputs for the n = z1 - z0 kept slices, each
 * optional (null = not wanted), dense [n][S][S]:
 *   img_f32  float32((img - min)/(max - min)), the division in float64 as numpy does           T1:296, 337
 *   img_u8   np.uint8(img * 255) of that float64 image (truncation; NaN -> 0)                   T1:165, 363
 *   lung_u8  img[img > 0] = 1 -> np.uint8(img * 255)                                            T1:341 + 213
 *   uniform  int32 [n]: 1 where np.unique(slice).size == 1 on the slice BEFORE the resize       T1:333
 *   minmax   double [n][2]: the resized image's min and max
 * A slice whose resized image has max == min gives what numpy gives: NaN in img_f32, 0 in both uint8 forms.
 * ws: unet_vol_slices_ws_bytes(n, S) bytes, 16-byte aligned; it starts with the resized float64 images [n][S][S] (tests read this stage).
 * Refusals, nothing launched (the same codes for unet_vol_unslice): a null vox / ws (canvas / mask / counts), X, Y, Z or S < 1, a datatype code outside the eight, a
 * voxel buffer off its item size, a workspace too small or off 16 bytes: UNET_E_ARG; a slice range that is empty or leaves [0, Z), S S or X Y >= 2^30: UNET_E_SHAPE. */
size_t unet_vol_slices_ws_bytes(int32_t n, int32_t S);
int32_t unet_vol_slices_f64(unet_ctx*, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter, int32_t z0,
                            int32_t z1, int32_t S, float* img_f32, uint8_t* img_u8, uint8_t* lung_u8, int32_t* uniform, double* minmax, void* ws, size_t ws_bytes,
                            void* stream);
/* The inverse of crop -> INTER_AREA resize to 125 x 250 -> fuse -> INTER_LINEAR resize to d x d (T1:352-358, 486): prob [n][d][d] (the model's output) -> canvas
 * [n][S][S].  rects: HOST array [n][2][4] = (x, y, w, h) of the two lung rectangles per slice (w <= 0 or h <= 0: absent), or NULL.  A canvas pixel (r, c) inside
 * rectangle k takes the bilinear sample (half-pixel centres, clamped to the edge, coordinates in float64, blend in float32 as top = p00 + (p01 - p00) fx, bot likewise,
 * value = top + (bot - top) fy, every operation rounded on its own) of prob at u' = (u + 0.5) d / 250 - 0.5, v' = (v + 0.5) d / 250 - 0.5 with u = (c - x + 0.5) 125 / w - 0.5 + 125 k,
 * v = (r - y + 0.5) 250 / h - 0.5; both rectangles: the larger value; neither: 0.  A slice without rectangles (it fell through uncropped, T1:347) is sampled
 * over the whole canvas: u' = (c + 0.5) d / S - 0.5. */
int32_t unet_vol_paste_back(unet_ctx*, const float* prob, int32_t n, int32_t d, const int32_t* rects, float* canvas, int32_t S, void* stream);
/* canvas [z1 - z0][S][S] -> patient space: resampled to [Y, X] with the same sampler, np.rot90 undone, mask[x + X (y + Y z)] = p > threshold (uint8, Fortran
 * order [X, Y, Z]; the slices outside [z0, z1) are set to 0) and counts[z - z0] = set voxels of slice z (int64 [z1 - z0]; integer sums: exact, the same on every run). */
int32_t unet_vol_unslice(unet_ctx*, const float* canvas, int32_t S, float threshold, int32_t X, int32_t Y, int32_t Z, int32_t z0, int32_t z1, uint8_t* mask,
                         int64_t* counts, void* stream);

/* ---- connected components of a mask volume (csrc/kernels_components.hip; exact against tests/components_oracle.py and scikit-image's label) ----
 * mask: uint8 [X, Y, Z] in Fortran order (x fastest: what unet_vol_unslice writes), foreground = non-zero.  connectivity 1, 2, 3 = 6, 18, 26 neighbours
 * (scikit-image's `connectivity=` of a 3-D array); anything else: UNET_E_ARG.  labels: int32, same layout, 16-byte aligned; 0 on the background, the components
 * numbered 1..n in ascending order of the C-order index (x Y + y) Z + z of their first voxel -- element for element `skimage.measure.label(mask != 0,
 * connectivity=c)` and `scipy.ndimage.label(mask, generate_binary_structure(3, c))`.  n_out: device int32, the number of components.  X Y Z < 2^31 (otherwise
 * UNET_E_ARG, nothing launched); a volume with a zero dimension gives n = 0 and touches nothing else.  ws: unet_vol_label_ws_bytes(X, Y, Z) bytes, 16-byte
 * aligned (one flag byte per voxel + the prefix sum's chunk totals).  Seven launches, each a phase of a union-find on C-order keys (brick-local in LDS, merge
 * across brick faces, flatten, count / scan / number the roots, final labels); integer arithmetic only: the same result on every run. */
size_t unet_vol_label_ws_bytes(int32_t X, int32_t Y, int32_t Z);
int32_t unet_vol_label(unet_ctx*, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t connectivity, int32_t* labels, int32_t* n_out, void* ws, size_t ws_bytes,
                       void* stream);
/* The same inside every axial slice: two voxels are neighbours only when dz = 0; connectivity 1, 2 = 4, 8 neighbours (anything else: UNET_E_ARG).  Contract, workspace
 * (unet_vol_label_ws_bytes) and numbering rule are unet_vol_label's: element for element scipy.ndimage.label(mask, s) with s = generate_binary_structure(3, c) whose
 * z = -1 and z = +1 planes are cleared. */
int32_t unet_vol_label_planar(unet_ctx*, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t connectivity, int32_t* labels, int32_t* n_out, void* ws,
                              size_t ws_bytes, void* stream);
/* Per component, one pass with integer atomics (summed per lane and per wave first): stats = n records of 64 bytes, record i for label i + 1:
 *   int64 count, sum_x, sum_y, sum_z;  int32 x0, x1, y0, y1, z0, z1 (inclusive bounding box), 2 x int32 padding.
 * The centroid is the caller's sum / count.  labels 16-byte aligned, stats 8-byte aligned; a label outside 1..n is ignored. */
int32_t unet_vol_component_stats(unet_ctx*, const int32_t* labels, int32_t X, int32_t Y, int32_t Z, int32_t n, void* stats, void* stream);
/* mask[v] = keep[labels[v]] ? 1 : 0 over the whole volume (keep: device uint8 [n + 1], keep[0] = 0 for the background; a label outside 0..n is dropped) and
 * counts[z - z0] = set voxels of slice z for z in [z0, z1) (int64, as unet_vol_unslice reports them). */
int32_t unet_vol_filter_components(unet_ctx*, const int32_t* labels, const uint8_t* keep, int32_t n, int32_t X, int32_t Y, int32_t Z, int32_t z0, int32_t z1, uint8_t* mask,
                                   int64_t* counts, void* stream);

/* ---- a mask volume against its ground truth (csrc/kernels_volscore.hip; exact against tests/volscore_oracle.py) ----
 * All volumes: [X, Y, Z] in Fortran order, X Y Z < 2^31 (otherwise UNET_E_ARG, nothing launched); a mask's foreground = non-zero.
 * counts[z][3] = int64 {tp, fp, fn} of slice z (pred & truth, pred & ~truth, truth & ~pred): integer sums per lane, per wave, then one atomic per workgroup and
 * slice; exact and the same on every run. */
int32_t unet_vol_confusion(unet_ctx*, const uint8_t* pred, const uint8_t* truth, int32_t X, int32_t Y, int32_t Z, int64_t* counts, void* stream);
/* surface[v] = mask[v] != 0 and some neighbour of v within the structuring element (connectivity 1, 2, 3 = 6, 18, 26 neighbours; anything else UNET_E_ARG) is
 * background; voxels outside the volume are background.  Element for element m ^ scipy.ndimage.binary_erosion(m, generate_binary_structure(3, c)) (border_value 0),
 * as uint8 0 / 1; surface must not be the mask's own buffer.  count: device int64, the number of surface voxels. */
int32_t unet_vol_surface(unet_ctx*, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t connectivity, uint8_t* surface, int64_t* count, void* stream);
/* Exact squared Euclidean distance transform.  The features are the non-zero voxels of vol (features_nonzero != 0) or its zero voxels (== 0); w = HOST pointer to
 * (sx^2, sy^2, sz^2), positive and finite, squared by the caller in float64.  For every voxel
 *     d2[v] = min over features f of fl( fl( fl(wx i^2) + fl(wy j^2) ) + fl(wz k^2) ),    (i, j, k) = v - f,
 * every fl one IEEE double operation (i^2 is an exact integer; no fused multiply-add); +inf everywhere when there is no feature.  fl(a + c) is monotone in a, so
 * the minimum commutes with the rounding and three passes (x, y, z) that each take the TRUE minimum along their line give this value bit for bit; the passes scan
 * the whole line.  No dimension may exceed UNET_VOL_EDT_MAX_DIM (UNET_E_ARG, nothing launched); a volume with a zero dimension touches nothing.  The passes run
 * in place in d2 (8-byte aligned): unet_vol_edt_ws_bytes is 0 today and ws may be null. */
#define UNET_VOL_EDT_MAX_DIM 4096
size_t unet_vol_edt_ws_bytes(int32_t X, int32_t Y, int32_t Z);
int32_t unet_vol_edt_sq(unet_ctx*, const uint8_t* vol, int32_t X, int32_t Y, int32_t Z, int32_t features_nonzero, const double* w, double* d2, void* ws, size_t ws_bytes,
                        void* stream);
/* x[i] = sqrt(x[i]) in place, n doubles. */
int32_t unet_vol_sqrt_f64(unet_ctx*, double* x, int64_t n, void* stream);
/* Over the voxels of the byte volume `surface` that are non-zero: result (device, 24 bytes, 8-byte aligned) = { int64 count, double max d2 (exact; 0 when count = 0),
 * double sum of sqrt(d2) }, and the d2 values themselves in gathered[0 .. min(count, capacity)) in no particular order (they are sorted afterwards).
 * ws: UNET_VOL_SURFDIST_WS_BYTES bytes, 8-byte aligned.  The sum has a fixed shape and uses no floating-point atomics, so it is the same on every run:
 *   items = ceil(N / 16), G = min(ceil(items / 256), UNET_VOL_SURFDIST_WS_BYTES / 8) workgroups of 256 lanes;
 *   a lane adds its voxels one by one: a chain of at most 16 ceil(items / (256 G)) additions; a 6-level butterfly over the 64 lanes of a wave; the 4 wave sums left to
 *   right (3 additions); a second launch of ONE workgroup: a chain of ceil(G / 256) partial sums per lane, the same butterfly, the same 3 additions.
 * The longest chain of additions behind the sum is therefore 16 ceil(items / (256 G)) + ceil(G / 256) + 18. */
#define UNET_VOL_SURFDIST_WS_BYTES 32768
int32_t unet_vol_surface_distances(unet_ctx*, const uint8_t* surface, const double* d2, int32_t X, int32_t Y, int32_t Z, void* result, double* gathered, int64_t capacity,
                                   void* ws, size_t ws_bytes, void* stream);
/* Two label volumes of unet_vol_label with n_t and n_p components: cover_t[i] = voxels of truth component i + 1 where labels_p is non-zero, cover_p[j] = voxels of
 * predicted component j + 1 where labels_t is non-zero (device int64; integer atomics, summed per lane and per wave first).  A label outside 1..n is ignored. */
int32_t unet_vol_lesion_overlap(unet_ctx*, const int32_t* labels_t, int32_t n_t, const int32_t* labels_p, int32_t n_p, int32_t X, int32_t Y, int32_t Z, int64_t* cover_t,
                                int64_t* cover_p, void* stream);

/* ---- binary morphology of a mask volume (csrc/kernels_morph.hip; exact against tests/morph_oracle.py and scipy.ndimage) ----
 * All volumes: [X, Y, Z] in Fortran order, X Y Z < 2^31; a mask's foreground = non-zero; results are uint8 0 / 1.  Every refusal is UNET_E_ARG with nothing launched; a
 * volume with a zero dimension touches nothing.  counts (nullable): device int64 [Z], 8-byte aligned, the set voxels of every slice of the result, as unet_vol_unslice
 * reports them (integer sums: exact, the same on every run).
 *
 * unet_vol_morph: op on the structuring element s = generate_binary_structure(3, connectivity) (connectivity 1, 2, 3 = 6, 18, 26 neighbours + the centre), or, with
 * planar != 0, s with its z = -1 and z = +1 planes cleared (connectivity 1, 2 only: every axial slice is processed on its own).  One step:
 *     dilate:  out[v] = OR over o in s of m[v + o]          erode:  out[v] = AND over o in s of m[v + o]
 * where m outside the volume is border_value (0 or 1) at EVERY step -- scipy.ndimage.binary_dilation / binary_erosion(mask, s, iterations, border_value=b).
 *     UNET_MORPH_DILATE / _ERODE: `iterations` steps;  _OPEN: `iterations` erosions then as many dilations;  _CLOSE: dilations then erosions, all with the same
 * border_value -- scipy.ndimage.binary_opening / binary_closing(mask, s, iterations, border_value=b).  iterations outside 1..UNET_VOL_MORPH_MAX_ITERATIONS, another op,
 * connectivity or border_value: UNET_E_ARG.  out (X Y Z bytes) must not overlap the mask.  ws: unet_vol_morph_ws_bytes(X, Y, Z) bytes, 16-byte aligned: two volumes of
 * one bit per voxel (rows padded to 64 voxels).  The byte volume is read once (pack) and written once (unpack, with the counts); each step is one launch over the packed
 * words: 2 + steps launches.  X need not be a multiple of anything (a multiple of 16 with 16-byte aligned buffers takes the 16-byte path). */
enum { UNET_MORPH_DILATE = 0, UNET_MORPH_ERODE = 1, UNET_MORPH_OPEN = 2, UNET_MORPH_CLOSE = 3 };
#define UNET_VOL_MORPH_MAX_ITERATIONS 64
size_t unet_vol_morph_ws_bytes(int32_t X, int32_t Y, int32_t Z);
int32_t unet_vol_morph(unet_ctx*, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t op, int32_t connectivity, int32_t planar, int32_t iterations,
                       int32_t border_value, uint8_t* out, int64_t* counts, void* ws, size_t ws_bytes, void* stream);
/* out[v] = d2[v] <= r2 (keep_le != 0) or d2[v] > r2 (keep_le == 0), d2 the result of unet_vol_edt_sq (X Y Z doubles), r2 = fl(r r) squared by the caller in float64,
 * finite and >= 0.  With d2 = the distance to the mask's foreground, `<=` is the dilation of the mask by the closed ball of radius r in the unit of the transform's
 * weights; with d2 = the distance to the mask's background, `>` is its erosion by that ball; both exact by the definition of d2.  The transform has no feature outside
 * the volume: the erosion treats the outside as FOREGROUND (a mask without background is kept whole), the dilation as background.  out must not overlap d2. */
int32_t unet_vol_ball(unet_ctx*, const double* d2, int32_t X, int32_t Y, int32_t Z, double r2, int32_t keep_le, uint8_t* out, int64_t* counts, void* stream);
/* scipy.ndimage.binary_fill_holes(mask, s), s as for unet_vol_morph (connectivity 1..3, or planar with 1..2): out = mask | every component of the mask's ZERO voxels
 * under s's connectivity that holds no voxel of the border -- the six faces of the volume, or, planar, the four edges of each slice.  The components are unet_vol_label's
 * (unet_vol_label_planar's) of the complement; one pass over the faces marks the labels found there (same-value byte stores); a last pass writes out and the counts.
 * Nothing iterates until stable: 7 + 2 launches whatever the mask.  out must not overlap the mask.  ws: unet_vol_fill_holes_ws_bytes(X, Y, Z) bytes, 16-byte aligned
 * (the labels, one byte per possible label, the label workspace: about 7 bytes per voxel). */
size_t unet_vol_fill_holes_ws_bytes(int32_t X, int32_t Y, int32_t Z);
int32_t unet_vol_fill_holes(unet_ctx*, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t connectivity, int32_t planar, uint8_t* out, int64_t* counts, void* ws,
                            size_t ws_bytes, void* stream);

/* ---- several models and test-time symmetries on one volume (csrc/kernels_ensemble.hip; bit-exact against tests/ensemble_oracle.py) ----
 * Every entry point checks its arguments first and refuses a bad one with UNET_E_ARG and nothing launched; a zero-sized input (n d d = 0, count = 0, nvox = 0,
 * X Y Z = 0) is a no-op that returns UNET_OK.  Volumes: [X, Y, Z] in Fortran order, X Y Z < 2^31.  All launches go to the caller's stream.
 *
 * unet_vol_dihedral: src, dst float32 [n][d][d] (dst must not overlap src); `code` is one of the eight symmetries of the square, by their numpy meaning on axes (1, 2):
 *     0 id   1 rot90 = np.rot90(a, 1, (1, 2))   2 rot180   3 rot270   4 hflip = a[:, :, ::-1]   5 vflip = a[:, ::-1, :]   6 transpose = a.swapaxes(1, 2)
 *     7 antitranspose = rot180 of the transpose.
 * A copy of 32-bit words: bit-exact, NaN payloads and signed zeros included.  Codes 1, 3, 6, 7 go through a 32 x 33 LDS tile, so both the reads and the writes run along
 * rows.  The inverse is the same call with the inverse code (1 <-> 3, every other code is its own inverse): the caller owns that table (volume.DIHEDRAL_INVERSE). */
int32_t unet_vol_dihedral(unet_ctx*, const float* src, int32_t n, int32_t d, int32_t code, float* dst, void* stream);
/* acc[i] = first ? fl(w c[i]) : fl(acc[i] + fl(w c[i])) for i < count: the product and the sum are rounded on their own (no fused multiply-add), so a numpy float32 loop
 * that adds the members in the same order gives the same bits.  acc must not overlap the canvas. */
int32_t unet_vol_canvas_axpy(unet_ctx*, const float* canvas, float w, float* acc, int64_t count, int32_t first, void* stream);
/* acc[i] = fl(acc[i] / denom) in place: the correctly rounded float32 quotient (x / 1 = x). */
int32_t unet_vol_canvas_div(unet_ctx*, float* acc, float denom, int64_t count, void* stream);
/* canvas [z1 - z0][S][S] -> prob float32 [X, Y, Z] (Fortran order), 0 outside [z0, z1): geometry and sampler of unet_vol_unslice without the comparison.  Both kernels
 * call one device function (csrc/vol_sample.h), so prob[v] > t is unet_vol_unslice's mask[v] for every t, element for element. */
int32_t unet_vol_unslice_prob(unet_ctx*, const float* canvas, int32_t S, int32_t X, int32_t Y, int32_t Z, int32_t z0, int32_t z1, float* prob, void* stream);
/* words: uint32 per voxel.  Bit `member` (0..31) of words[v] = mask[v] != 0; first != 0 overwrites the word (the other bits become 0), otherwise the bit is OR-ed in. */
int32_t unet_vol_vote_pack(unet_ctx*, const uint8_t* mask, int32_t member, int32_t first, uint32_t* words, int64_t nvox, void* stream);
/* The vote words of M members (1..32; bits at or above M are a caller error and take no part) -> with v = popcount(words[.]):
 *   mask           uint8, unet_vol_unslice's layout: v >= min_votes (1 <= min_votes <= M)
 *   votes          uint8: v; may be NULL
 *   counts         int64 [Z]: the set voxels of mask per slice
 *   member_voxels  int64 [M]: the voxels member m marked
 *   pair           int64 [M][M]: the voxels members a and b both marked; symmetric, its diagonal is member_voxels
 *   hist           int64 [M + 1]: the voxels with k votes
 * Integer sums only: exact and the same on every run.  One lane per voxel; a wave adds from ballots: the consensus bit for counts, one ballot per vote count present for
 * hist, and for pair, for every bit a with a non-empty ballot and every b >= a, the popcount of the ballot of (w >> a) & (w >> b) & 1.  A wave whose words are all zero
 * writes its zeros and is otherwise skipped.  Sums are int32 in LDS per workgroup (a workgroup sees fewer than 2^31 voxels) and leave it as one 64-bit atomic per non-zero
 * entry; the grid is bounded (at most 2048 workgroups) and strides over the slices and inside them.  A second launch of one workgroup mirrors pair and copies its diagonal. */
int32_t unet_vol_vote_reduce(unet_ctx*, const uint32_t* words, int32_t M, int32_t X, int32_t Y, int32_t Z, int32_t min_votes, uint8_t* mask, uint8_t* votes,
                             int64_t* counts, int64_t* member_voxels, int64_t* pair, int64_t* hist, void* stream);

/* ---- what the CT holds under a mask (csrc/kernels_intensity.hip; exact against tests/intensity_oracle.py) ----
 * vox, dtype, X, Y, Z, scaled, slope, inter: the uploaded volume of unet_vol_slices_f64 (Fortran order [X, Y, Z], native byte order, one of the eight NIfTI codes).  The
 * value of voxel v is get_fdata()'s: float64(raw), then, when scaled != 0, (. * slope) + inter as two rounded operations.  Groups: exactly one of `labels` (int32, same
 * layout) and `mask` (uint8, non-zero = group 1) is non-null.  A voxel takes part when its group g lies in 1..n and `region` (uint8, same layout, nullable) is non-zero
 * there; a label outside 1..n is ignored.  A NaN value takes part only in the NaN column.  X Y Z >= 2^31, an unknown dtype, both or neither of labels / mask, n < 0:
 * UNET_E_ARG and nothing is launched.  A volume with a zero dimension returns UNET_OK with the outputs in their empty state (counts 0, min / max (+inf, -inf)).
 *
 * unet_vol_intensity_bands: `edges` is a HOST array of n_edges doubles, finite and strictly ascending, 1 <= n_edges <= UNET_VOL_INTENSITY_MAX_EDGES (anything else:
 * UNET_E_ARG).  B = n_edges + 1 bands; band b of a non-NaN value v = the number of edges <= v = np.searchsorted(edges, v, side="right").
 *   band_counts   device int64 [n][B + 1]: the voxels of group g + 1 in every band; column B counts its NaN voxels
 *   slice_counts  device int64 [Z][B + 1]: the same over all taking-part voxels of a slice; nullable
 *   minmax        device double [n][2]: the exact minimum and maximum of the group's non-NaN values (-0.0 orders below +0.0), (+inf, -inf) for a group without one; nullable
 * All three are overwritten: the caller does not zero them.  All 8-byte aligned.  Integer sums (per wave by ballot, per workgroup in an LDS table while n (B + 1) <= 4096
 * and n <= 1024, 64-bit atomics beyond) and min / max only: the same bits on every run, for any n >= 0 and any mix of groups inside a wave. */
#define UNET_VOL_INTENSITY_MAX_EDGES 63
int32_t unet_vol_intensity_bands(unet_ctx*, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter,
                                 const int32_t* labels, const uint8_t* mask, int32_t n, const uint8_t* region, const double* edges, int32_t n_edges, int64_t* band_counts,
                                 int64_t* slice_counts, double* minmax, void* stream);
/* The taking-part non-NaN voxels, compacted: values[k] (double) and groups[k] (int32 1..n; nullable) for k < min(count, capacity), in no particular order (they are sorted
 * afterwards).  count: device int64, the number of such voxels whatever the capacity; when it exceeds `capacity`, exactly `capacity` pairs are written and nothing past
 * them (unet_vol_surface_distances's rule). */
int32_t unet_vol_intensity_gather(unet_ctx*, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter,
                                  const int32_t* labels, const uint8_t* mask, int32_t n, const uint8_t* region, double* values, int32_t* groups, int64_t capacity,
                                  int64_t* count, void* stream);
/* values: device doubles already ordered by (group, value ascending); offsets: device int64 [n + 1], offsets[0] = 0, non-decreasing, offsets[n] = total: group g's run is
 * values[offsets[g] .. offsets[g + 1]).  out: device double [n][2] = (sum, ssd) of every run v_0 .. v_{m-1}:
 *   partial_c = the left-to-right float64 sum of v[256 c .. min(256 c + 256, m) - 1], starting from its first element (np.cumsum(chunk)[-1]);
 *   sum = the left-to-right sum of the partials;  mean = sum / m;
 *   ssd = the same two-level sum over q_i = fl(d_i d_i), d_i = fl(v_i - mean).
 * An empty group gives (0, 0).  The order is canonical and the tree fixed (no fused multiply-add, no floating-point atomics): bit-identical from run to run.
 * ws: unet_vol_group_moments_ws_bytes(total, n) bytes, 8-byte aligned (the means and one partial sum per 256-element chunk); nothing is written past ws_bytes. */
size_t unet_vol_group_moments_ws_bytes(int64_t total, int32_t n);
int32_t unet_vol_group_moments(unet_ctx*, const double* values, const int64_t* offsets, int32_t n, double* out, void* ws, size_t ws_bytes, void* stream);

/* ---- left and right lung (csrc/kernels_lungside.hip; exact against tests/lungside_oracle.py) ----
 * All volumes: [X, Y, Z] in Fortran order, X Y Z < 2^31 (otherwise UNET_E_ARG, nothing launched); a volume with a zero dimension returns UNET_OK and touches nothing,
 * the outputs included.  Integer arithmetic only (the distances are compared as order-preserving 64-bit keys of their bit patterns, which is value order for the
 * non-negative values and +inf that unet_vol_edt_sq writes); integer sums per lane, per wave and per workgroup, then 64-bit atomics: the same bits on every run.
 *
 * unet_vol_side_assign: mask uint8 (non-zero = lung), d2_a / d2_b the results of unet_vol_edt_sq to the voxels of seed a / seed b (X Y Z doubles each, 8-byte aligned),
 * side_a, side_b = 1 and 2 in either order (anything else: UNET_E_ARG).  sides (uint8, X Y Z bytes, not the mask's own buffer):
 *     sides[v] = 0 where mask[v] == 0, else the side of the seed with the smaller distance; on a tie the seed whose side is 1 -- whichever of a, b that is.
 * counts: device int64 [3], 8-byte aligned, overwritten: the voxels of sides holding 0, 1, 2 (summed per lane and per wave, one atomic per workgroup and entry).
 * 17 bytes read and 1 written per voxel: a lane takes four voxels with one 4-byte mask load, two 16-byte loads per distance stream and one 4-byte store when mask /
 * sides are 4-byte and d2_a / d2_b 16-byte aligned (one voxel per lane otherwise); a wave whose mask bytes are all zero reads no distance. */
int32_t unet_vol_side_assign(unet_ctx*, const uint8_t* mask, const double* d2_a, const double* d2_b, int32_t X, int32_t Y, int32_t Z, int32_t side_a, int32_t side_b,
                             uint8_t* sides, int64_t* counts, void* stream);
/* sides: uint8 0 / 1 / 2 (a value above 2 counts as 0); infection: uint8, non-zero = infected, nullable (nothing is infected); labels: int32, lesions 1..n, nullable, 4-byte
 * aligned; a label outside 1..n is ignored, never an address.  n < 0: UNET_E_ARG.  All outputs are device int64, 8-byte aligned and overwritten (the caller does not zero them):
 *   totals       [2][3]  row 0: the voxels of sides by value; row 1: the voxels with infection != 0 by the side value under them (column 0: infected outside both lungs)
 *   lesion_side  [n][3]  the voxels of lesion i + 1 by side value (all zero without labels); may be null when n == 0
 *   per_slice    [Z][6]  {lung L, lung R, infected outside, infected L, infected R, 0} of every slice; nullable
 * One lane per voxel; a wave counts the five slice columns with ballots, and the lanes that share a (lesion, side) key with one ballot whose first lane adds the popcount
 * (one add per distinct key of a wave) -- to a table in LDS while 3 n <= 4096, flushed once per workgroup with 64-bit atomics, straight to lesion_side beyond that.  The
 * slice counters sit in LDS and leave when the workgroup's slice changes. */
int32_t unet_vol_side_table(unet_ctx*, const uint8_t* sides, const uint8_t* infection, const int32_t* labels, int32_t n, int32_t X, int32_t Y, int32_t Z, int64_t* totals,
                            int64_t* lesion_side, int64_t* per_slice, void* stream);

/* ---- a picture of a segmented CT volume (csrc/kernels_render.hip; volume.project_volume / render_planes) ----
 * The volume is described as for unet_vol_intensity_bands: vox / dtype / X, Y, Z / scaled, slope, inter, decoded as get_fdata() decodes it ((float64(v) * slope) + inter).
 * Label volumes are uint8 (datatype code 2) or int32 (code 8, 4-byte aligned) of the same shape, device buffers in Fortran order.
 *
 * unet_vol_project: the slab [a, b) of `axis` (0, 1, 2) collapsed into one plane.  plane: device float64, 8-byte aligned, one element per column -- the largest (mode 0)
 * or smallest (mode 1) decoded value of the column, NaN voxels skipped, NaN for a column of NaNs only (-0.0 orders below +0.0): np.fmax.reduce / np.fmin.reduce.  The plane
 * of axis 0, 1, 2 is laid out as a Fortran-order volume of shape [1, Y, Z], [X, 1, Z], [X, Y, 1] and can be handed to unet_vol_render with datatype code 64.
 * labels / label_dtypes / label_planes: HOST arrays of n_labels (0..UNET_RENDER_MAX_LAYERS) device pointers / datatype codes / device output pointers; plane l receives
 * the largest label of every column in the element type of volume l; a null labels[l] is skipped.  Both results are independent of the order of the walk.
 * Along y or z one lane owns an x and walks the slab; along x one wave owns a column, its lanes stride x and meet in a __shfl_xor butterfly: every load is coalesced.
 * UNET_E_ARG: axis outside 0..2, a >= b, a slab that leaves the axis, mode outside 0..1, more than UNET_RENDER_MAX_LAYERS label volumes, a volume without voxels. */
#define UNET_RENDER_MAX_TILES 64
#define UNET_RENDER_MAX_LAYERS 4
int32_t unet_vol_project(unet_ctx*, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter, int32_t axis, int32_t a,
                         int32_t b, int32_t mode, const void* const* labels, const int32_t* label_dtypes, void* const* label_planes, int32_t n_labels, double* plane,
                         void* stream);
/* One tile of a canvas: plane `index` of `axis` (a voxel index of the volume, inside the region), drawn w x h pixels with its top-left corner at canvas pixel (x0, y0). */
typedef struct unet_render_tile { int32_t axis, index, x0, y0, w, h; } unet_render_tile;
/* One overlay: labels (device; dtype 2 = uint8, 8 = int32), palette (device uint8 [palette_size][3], palette_size >= 2), the alphas 0..255 of its inside and its outline. */
typedef struct unet_render_layer { const void* labels; const uint8_t* palette; int32_t dtype, palette_size, fill_alpha, outline_alpha; } unet_render_layer;
/* unet_vol_render: canvas = device uint8 [H][W][3] (RGB), H <= 65535, H W 3 < 2^31.  tiles (up to UNET_RENDER_MAX_TILES) and layers (up to UNET_RENDER_MAX_LAYERS) are
 * HOST arrays: they are checked on the host before anything is launched and travel in the kernel arguments (no copy).  roi: host int32 [6] = x_lo, x_hi, y_lo, y_hi,
 * z_lo, z_hi, the region of the volume that is shown, with extents n_x, n_y, n_z; table: device uint8 [256][3]; background: 0xRRGGBB.
 *   geometry   image row i runs against the second in-plane axis, column j along the first (np.rot90 of the slice): axial (axis 2) (x = j, y = n_y - 1 - i), coronal
 *              (axis 1) (x = j, z = n_z - 1 - i), sagittal (axis 0) (y = j, z = n_z - 1 - i), region coordinates
 *   sample     float64, half-pixel centres: u = (j + 0.5) n_u / w - 0.5, v = (i + 0.5) n_v / h - 0.5.  interp 0: the voxel min(int(floor((j + 0.5) n_u / w)), n_u - 1);
 *              interp 1: the four neighbours floor(u), floor(u) + 1 (likewise v) clamped to the region, fx = u - floor(u), top = p00 + (p01 - p00) fx,
 *              bot = p10 + (p11 - p10) fx, val = top + (bot - top) fy, every operation rounded on its own.  Labels are always sampled as interp 0 samples.
 *   grey       t = (val - lo) / (hi - lo); g = 0 when t <= 0 or val is NaN, 255 when t >= 1, else (int)floor(t 255 + 0.5); the pixel starts as table[g]
 *   layers     in order: a sampled label L <= 0 leaves the pixel; else colour = palette[1 + (L - 1) % (palette_size - 1)], alpha = outline_alpha when one of the four
 *              neighbouring pixels OF THE TILE samples another label (outside the tile: 0), fill_alpha otherwise; channel = (colour alpha + channel (255 - alpha) + 127) / 255
 *   elsewhere  fill_background != 0: the canvas pixels no tile covers take the background (the caller does not clear the canvas); 0: they are left as they are, so that
 *              several calls can draw on one canvas
 * UNET_E_ARG before any launch: more than 64 tiles or 4 layers, an axis or index outside the region, w < 1 or h < 1, a tile that leaves the canvas, two tiles that
 * overlap, an empty region or one that leaves the volume, hi <= lo or a NaN window, interp outside 0..1, palette_size < 2, an alpha outside 0..255, a null layer. */
int32_t unet_vol_render(unet_ctx*, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter, const int32_t* roi,
                        double lo, double hi, const uint8_t* table, int32_t interp, int32_t background, int32_t fill_background, const unet_render_layer* layers,
                        int32_t n_layers, const unet_render_tile* tiles, int32_t n_tiles, uint8_t* canvas, int32_t H, int32_t W, void* stream);

/* ---- a volume on another grid (csrc/kernels_resample.hip; new: the reference never leaves the grid of the file) -------------------------------
 * Source [X, Y, Z] and output [X2, Y2, Z2] are device volumes in Fortran order.  M: HOST, 12 finite doubles, row-major 3 x 4: output voxel (i, j, k) looks at the source
 * coordinate s_r = ((M[r][0] i + M[r][1] j) + M[r][2] k) + M[r][3], float64, every operation rounded on its own.  mode 0 = "nearest" (the edge voxel repeats), 1 =
 * "constant" (outside reads cval; scipy.ndimage's grid-constant).  A coordinate is compared as a double before anything is converted to an integer: entries of 1e300
 * are safe; a coordinate that overflows to +-inf is clamped (mode 0) or outside (mode 1) like any other, and a NaN coordinate (inf - inf of an M that overflows) counts as 0
 * in mode 0 and as outside in mode 1: both entry points then write cval (the linear one takes the weight 0 on an axis whose two neighbours are both outside).
 * UNET_E_ARG before any launch, the output untouched: a non-finite entry of M, an output extent < 1, X Y Z >= 2^31 on either side, a negative source extent, mode outside
 * 0..1, an unknown dtype / dst_dtype / element size, a null or misaligned buffer, a source without voxels in mode 0.  A source with a zero extent (whatever its other
 * two extents are) fills the output with cval in mode 1.
 *   unet_vol_resample_nearest  elements of elem_bytes = 1, 2, 4 or 8 bytes, moved untouched: q_r = floor(s_r + 0.5); mode 0 clamps q_r to [0, n_r - 1], mode 1 writes the
 *                              low elem_bytes bytes of cval_bits where any q_r is outside.
 *   unet_vol_resample_linear   the source is described and decoded as for unet_vol_intensity_bands ((float64(v) slope) + inter when scaled); cval is a decoded value.
 *                              Mode 0 first clamps s_r to [0, n_r - 1].  f = floor(s), t = s - f; the eight neighbours f, f + 1 per axis are clamped to the volume
 *                              (mode 0) or read cval outside it (mode 1); lerp(a, b, w) = a + (b - a) w along x (c00 = lerp(p000, p100, tx), c10 at y + 1, c01 at z + 1,
 *                              c11), then y (lerp(c00, c10, ty), lerp(c01, c11, ty)), then z.  NaN and +-inf propagate as IEEE says: a NaN neighbour makes the output
 *                              NaN even at weight 0, as scipy.ndimage does.  dst_dtype 64 = that float64, 16 = it rounded once to float32, 2 = uint8 (result >= 0.5):
 *                              a 0 / 1 mask resampled smoothly. */
int32_t unet_vol_resample_nearest(unet_ctx*, const void* src, int32_t elem_bytes, int32_t X, int32_t Y, int32_t Z, const double* M, int32_t mode, uint64_t cval_bits,
                                  void* dst, int32_t X2, int32_t Y2, int32_t Z2, void* stream);
int32_t unet_vol_resample_linear(unet_ctx*, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter, const double* M,
                                 int32_t mode, double cval, void* dst, int32_t dst_dtype, int32_t X2, int32_t Y2, int32_t Z2, void* stream);

/* ---- the similarity of two volumes under candidate transforms (csrc/kernels_register.hip; new: the reference never compares two scans) --------
 * unet_vol_joint_hist: the joint intensity histogram of a fixed volume [X, Y, Z] and a moving volume [Xm, Ym, Zm] (device, Fortran order, each described and decoded
 * as for unet_vol_resample_linear: dtype, scaled, slope, inter) under K matrices at once.  M: HOST, K x 12 finite doubles, 1 <= K <= UNET_VOL_JOINT_HIST_MAX_K, each
 * row-major 3 x 4 in section 4w's convention: fixed voxel (i, j, k) looks at the moving coordinate s_r = ((M[r][0] i + M[r][1] j) + M[r][2] k) + M[r][3].  mask: uint8
 * on the fixed grid, or NULL.  A fixed voxel is counted for candidate c iff the mask is NULL or non-zero there, its decoded value is not NaN, every s_r satisfies
 * 0 <= s_r <= n_r - 1 compared as doubles (a NaN or inf coordinate is outside; entries of 1e300 are safe) and the moving sample is not NaN.  The moving sample is the
 * float64 unet_vol_resample_linear writes in mode 0 with dst_dtype 64 at that coordinate (f = floor(s), t = s - f, the upper neighbour clamped, lerp along x, y, z, one
 * rounding per operation; the two share their code).  bin(v) = floor((v - lo) scale), scale = bins / (hi - lo) computed once on the host in float64, the subtraction and
 * the product rounded separately; the product is compared as a double first: below 0 -> bin 0, >= bins -> bins - 1, so +-inf values clamp.  counts: device uint32
 * [K][bins][bins], fixed bin major; the entry point clears it, and the counts are exact integers whatever the order of accumulation.
 * UNET_E_ARG before any launch, counts untouched: K outside 1..16, bins outside 2..UNET_VOL_JOINT_HIST_MAX_BINS, a non-finite matrix entry or window, hi <= lo (or a
 * hi - lo that overflows), an unknown dtype, a null (fixed, moving, M, counts) or misaligned buffer, either volume with no voxels or with 2^31 or more. */
#define UNET_VOL_JOINT_HIST_MAX_K 16
#define UNET_VOL_JOINT_HIST_MAX_BINS 64
int32_t unet_vol_joint_hist(unet_ctx*, const void* fixed, int32_t f_dtype, int32_t X, int32_t Y, int32_t Z, int32_t f_scaled, double f_slope, double f_inter,
                            const uint8_t* mask, const void* moving, int32_t m_dtype, int32_t Xm, int32_t Ym, int32_t Zm, int32_t m_scaled, double m_slope, double m_inter,
                            const double* M, int32_t K, int32_t bins, double f_lo, double f_hi, double m_lo, double m_hi, uint32_t* counts, void* stream);

/* ---- the deformable refinement of a registered follow-up (csrc/kernels_deform.hip; new: the reference never compares two scans) -----------------
 * A displacement field u lives on a field grid [Xf, Yf, Zf]: device float32 [3][Xf Yf Zf], component major, each component a volume in Fortran order (NIfTI code 16), in
 * millimetres of the fixed world frame.  A fixed world point p corresponds to the moving world point T (p + u(p)), T the rigid transform.  For a target voxel (i, j, k)
 * the moving voxel coordinate is s_r = ((c_r + L[r][0] u_0) + L[r][1] u_1) + L[r][2] u_2 with c_r = ((W[r][0] i + W[r][1] j) + W[r][2] k) + W[r][3] of section 4w.
 * W: HOST, 12 doubles, row-major 3 x 4 (inv(A_moving) T A_target); L: HOST, 9 doubles, row-major 3 x 3 ((inv(A_moving) T)[:3, :3]: millimetres -> moving voxels).  u is the
 * stored element when the target grid is the field grid, else the three components sampled trilinearly (vol_trilinear.h's blend, float64, not rounded) at the field
 * coordinate F (i, j, k) clamped into the field.  Every float64 operation is rounded on its own; a field element is rounded to float32 once, on store.  All host matrices
 * must be finite.  UNET_E_ARG before any launch, the outputs untouched: a null or misaligned buffer, an extent outside the ranges of unet_vol_resample_linear, an unknown
 * datatype code, a non-finite matrix entry, and what each entry names below.
 *   unet_vol_smooth_axis   dst <- one pass of a (2 R + 1)-tap filter along `axis` (0 = x, 1 = y, 2 = z) of C float32 volumes [X, Y, Z] stored one after the other (1 <= C
 *                          <= 1024): dst[p] = float32(sum_t weights[t] src[clamp(p + t - R, 0, n - 1)]) -- the edge voxel repeats --, the sum in float64 from 0 in
 *                          ascending t, acc + fl(w v).  weights: HOST, 2 R + 1 finite doubles (a normalised Gaussian, computed once by the caller), 0 <= R <=
 *                          UNET_VOL_SMOOTH_MAX_RADIUS; R = 0 with weight 1 is a copy.  src != dst.
 *   unet_vol_demons_step   field_out <- u + v, one launch, the warped image is never stored.  fixed [X, Y, Z] (the field grid) and moving [Xm, Ym, Zm] are described and
 *                          decoded as for unet_vol_resample_linear; mask: uint8 on the fixed grid, or NULL.  m_w = the moving sample at s (rs_blend_inside, as
 *                          unet_vol_joint_hist), d = f - m_w, g = Ginv (the index-space differences of f) with Ginv: HOST, 9 doubles, row-major inv(A_fixed[:3, :3])^T;
 *                          a difference is central ((f[p + 1] - f[p - 1]) 0.5), one-sided at a border (denominator 1) and 0 on an axis of extent 1.
 *                          v = d g / (|g|^2 + d^2 / delta^2), delta > 0 the step bound in mm (delta^2 computed once on the host); v = 0 where the mask byte is 0, f or
 *                          m_w is NaN, a coordinate is not within 0 <= s_r <= n_r - 1 (compared as doubles) or the denominator is not above 1e-9 (a NaN one is not).
 *                          field_in != field_out.
 *   unet_vol_warp_field    dst [X2, Y2, Z2] <- the source [X, Y, Z] at s.  field: [3][Xf Yf Zf]; F: HOST, 12 doubles, output voxel index -> field voxel coordinate, or
 *                          NULL: the field lies on the output grid and (Xf, Yf, Zf) must be (X2, Y2, Z2).  order 1: the blend of unet_vol_resample_linear (dtype, scaled,
 *                          slope, inter, mode, cval; dst_dtype 64, 16 or 2 = result >= 0.5); order 0: the stored element at floor(s + 0.5) moved untouched as in
 *                          unet_vol_resample_nearest (elements of the size of dtype, mode 1 writes the low bytes of cval_bits outside; dst_dtype = dtype).  With a field
 *                          of zeros the result is, bit for bit, that of unet_vol_resample_linear / _nearest with matrix W: the samplers are shared.
 *   unet_vol_jacobian      det <- float32(det(I + D Ainv)) per field voxel, D[c][a] the index-space difference of u_c along axis a (as the demons step takes those of
 *                          f), Ainv: HOST, 9 doubles, row-major inv(A_field[:3, :3]); the determinant by its first row, in float64.  folded: device uint32, cleared by
 *                          the entry point: the number of voxels whose float64 determinant is <= 0 (integer atomics; a NaN is not counted). */
#define UNET_VOL_SMOOTH_MAX_RADIUS 32
int32_t unet_vol_smooth_axis(unet_ctx*, const float* src, int32_t C, int32_t X, int32_t Y, int32_t Z, int32_t axis, int32_t R, const double* weights, float* dst,
                             void* stream);
int32_t unet_vol_demons_step(unet_ctx*, const void* fixed, int32_t f_dtype, int32_t X, int32_t Y, int32_t Z, int32_t f_scaled, double f_slope, double f_inter,
                             const uint8_t* mask, const void* moving, int32_t m_dtype, int32_t Xm, int32_t Ym, int32_t Zm, int32_t m_scaled, double m_slope, double m_inter,
                             const double* W, const double* L, const double* Ginv, double delta, const float* field_in, float* field_out, void* stream);
int32_t unet_vol_warp_field(unet_ctx*, const void* src, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter, const double* W,
                            const double* L, const float* field, int32_t Xf, int32_t Yf, int32_t Zf, const double* F, int32_t order, int32_t mode, double cval,
                            uint64_t cval_bits, void* dst, int32_t dst_dtype, int32_t X2, int32_t Y2, int32_t Z2, void* stream);
int32_t unet_vol_jacobian(unet_ctx*, const float* field, int32_t X, int32_t Y, int32_t Z, const double* Ainv, float* det, uint32_t* folded, void* stream);

/* ---- the surface of a mask, a label volume or a scalar volume as a triangle mesh (csrc/kernels_mesh.hip; bit-exact against tests/mesh_oracle.py) ----
 * Marching tetrahedra on the Freudenthal split of every lattice cell (six tetrahedra per cube, one per axis order; face diagonals agree between neighbouring cubes, so there
 * is no ambiguous case).  src: a volume [X, Y, Z] in Fortran order.  kind 0: a uint8 mask (dtype 2), inside = non-zero byte, any alignment; kind 1: int32 labels (dtype 8),
 * inside = label == select, or any non-zero label when select = 0; kind 2: a scalar volume of any of the eight NIfTI codes, decoded as unet_vol_resample_linear decodes it
 * (scaled, slope, inter), inside = value > iso (a NaN is outside, a value equal to iso is outside).  closed != 0 surrounds the volume with one layer of virtual outside
 * samples of value pad_value (finite, <= iso), so that a surface that touches the border is closed; the lattice is then [X + 2, Y + 2, Z + 2] and a virtual point lies at
 * voxel index -1 or n.  There is one vertex per crossed lattice edge, owned by the edge's lower endpoint q with an edge type 0..6 for the directions (1,0,0) (0,1,0) (0,0,1)
 * (1,1,0) (1,0,1) (0,1,1) (1,1,1); vertex id = rank of (q in Fortran order of the lattice, type); triangles are ordered by (cell, tetrahedron, table order) and wound so
 * that their normals point out of the inside.  The vertex of an edge lies at voxel coordinate q + t d: t = 0.5 for kinds 0 and 1 and for an edge with a non-finite endpoint,
 * else t = fl(fl(iso - a) / fl(b - a)), a the value at q and b at q + d; it is stored as float32(((m0 x + m1 y) + m2 z) + m3) per row of M (HOST, 12 doubles, row-major
 * 3 x 4: the grid's affine, or diag(pixdim)), every float64 operation rounded on its own.  group[t] = the label at the inside endpoint of triangle t's first edge (1 for
 * kinds 0 and 2).  UNET_E_ARG before any launch, the outputs untouched: a null or misaligned buffer (the volume to its element size, the workspace to 16 bytes, totals to 8,
 * the outputs to 4), an unknown kind or datatype code, a negative extent or a lattice of 2^31 points or more, a non-finite iso, pad_value or matrix entry, pad_value > iso,
 * select < 0, a workspace below unet_vol_mesh_ws_bytes, a capacity that is negative or 2^31 or more.  A volume with a zero dimension, or an unpadded one with an extent of 1
 * (no cells), gives totals (0, 0) and touches nothing else.
 *   unet_vol_mesh_count    fills ws (one flag byte per lattice point, bit e = edge type e is crossed and both ends exist; one byte per cell, 0..12 triangles; the chunk
 *                          offsets of both prefix sums) and totals: device int64 [2] = (vertices, triangles).  Integer arithmetic, no atomics: the same bits on every run.
 *   unet_vol_mesh_emit     the same volume, arguments and ws again, after the host has read totals (and refused 2^31 or more).  vertices: float32 [capacity_v][3];
 *                          triangles: int32 [capacity_t][3]; groups: int32 [capacity_t] or NULL.  With a capacity below the total exactly `capacity` items are written
 *                          and nothing past them (unet_vol_surface_distances's rule); a zero capacity writes none and its pointer may be NULL.
 *   unet_vol_mesh_measure  per triangle, in float64 from the stored float32 vertices a, b, c: area[t] = fl(0.5 sqrt((x_x^2 + x_y^2) + x_z^2)) with x = (b - a) x (c - a), each
 *                          component fl(fl(u_y v_z) - fl(u_z v_y)); signed_volume[t] = fl(((a_x n_x + a_y n_y) + a_z n_z) / 6) with n = b x c.  Either output may be NULL.  A
 *                          vertex index outside 0..nv - 1 is never an address: that triangle measures NaN.  The sums are the caller's (unet_vol_group_moments). */
size_t unet_vol_mesh_ws_bytes(int32_t X, int32_t Y, int32_t Z, int32_t closed);
int32_t unet_vol_mesh_count(unet_ctx*, const void* src, int32_t kind, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter, double iso,
                            int32_t select, int32_t closed, double pad_value, void* ws, size_t ws_bytes, int64_t* totals, void* stream);
int32_t unet_vol_mesh_emit(unet_ctx*, const void* src, int32_t kind, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter, double iso,
                           int32_t select, int32_t closed, double pad_value, const double* M, const void* ws, size_t ws_bytes, float* vertices, int64_t capacity_v,
                           int32_t* triangles, int32_t* groups, int64_t capacity_t, void* stream);
int32_t unet_vol_mesh_measure(unet_ctx*, const float* vertices, int64_t nv, const int32_t* triangles, int64_t nt, double* area, double* signed_volume, void* stream);

/* ---- every lesion from a baseline to its follow-up (csrc/kernels_track.hip; exact against tests/track_oracle.py; tracking.py) ----
 * labels_a, labels_b: two int32 label volumes [X, Y, Z] in Fortran order on ONE grid, 4-byte aligned, with lesions 1..n_a and 1..n_b (unet_vol_label); a label outside 0..n
 * counts as 0 and is never an address.  UNET_E_ARG before any launch, the outputs untouched: n_a or n_b negative, a negative extent or 2^31 voxels or more, a null or
 * misaligned buffer, and what each entry adds below.  A volume with a zero dimension is UNET_OK with the outputs in their empty state.  Integer arithmetic only; no
 * workgroup waits for another one; every sum is an integer that leaves as an integer atomic: the same bits on every run.  A lane takes four voxels with one 16-byte load per
 * volume when both label pointers are 16-byte aligned, voxel by voxel otherwise and in the last N % 4 voxels.
 *
 * unet_vol_label_pairs: the sparse contingency table.  The key of a voxel is ((uint64)a << 32) | (uint32)b; the pair (0, 0) is not counted (its key, 0, marks an empty slot),
 * (a, 0) and (0, b) are: the row and column sums of the table are the lesion sizes.  keys (uint64) and counts (int64) are an open-addressing table of `capacity` slots,
 * a power of two in 16 .. 2^30 (anything else: UNET_E_ARG), 8-byte aligned; keys, counts and info are cleared on the stream first.  A pair claims a slot with a 64-bit
 * compare-and-swap on keys and adds to counts[slot] with a 64-bit atomic; a slot's key is written once and never changes.  Probing is linear from the top bits of
 * key * 0x9E3779B97F4A7C15, at most `capacity` probes: a table loaded to exactly 1.0 completes, a full one never spins.
 *   info: device int64 [3] = occupied slots, voxels that found no slot (0: the table is complete), voxels with either label non-zero;
 *         sum(counts) + info[1] == info[2] always.
 * WHICH slot a pair lands in is unspecified (it depends on who claims first), and so is which pairs got in when the table overflows: callers sort by key, and call again
 * with a larger table when info[1] != 0.  A workgroup walks a contiguous range of chunks of UNET_VOL_PAIRS_CHUNK voxels and counts in an LDS table of
 * UNET_VOL_PAIRS_LDS_SLOTS slots first (64-bit key, 32-bit count, 16 probes; a pair that finds no slot there goes straight to the global table), flushed when its range ends.
 * The lanes of a wave that share the leading lane's pair are summed with shuffles and sent as one add (two rounds), the rest per lane.
 *
 * unet_vol_track_map: lut_a / lut_b (int32) and cls_a / cls_b (uint8) are DEVICE tables of n + 1 entries; entry 0 is read as 0 whatever it holds.  Per voxel
 *   track_a = lut_a[a], track_b = lut_b[b], cls = 3 where a > 0 and b > 0, cls_a[a] where only a > 0, cls_b[b] where only b > 0, 0 elsewhere.
 * cls (uint8, not a label volume's own buffer), track_a, track_b (int32) and per_slice may each be null -- a null output is not written -- but not all four (UNET_E_ARG); a
 * table may be null when no output reads it or its n is 0.  per_slice: int64 [Z][6], overwritten: the voxels of every class 0..5 per axial slice, summed per lane, per wave
 * (shuffles) and per workgroup in LDS, leaving as 64-bit atomics when the workgroup's slice changes.  A class value above 5 in entries 1..n of a class table is UNET_E_ARG:
 * when cls or per_slice is asked for, the entry point copies both class tables to the host and synchronises the stream before it writes anything. */
#define UNET_VOL_PAIRS_CHUNK 4096
#define UNET_VOL_PAIRS_LDS_SLOTS 1024
#define UNET_TRACK_CLS_NONE 0
#define UNET_TRACK_CLS_RESOLVED 1      /* a lesion of a alone that has no partner */
#define UNET_TRACK_CLS_SHRINKAGE 2     /* a alone, inside a lesion that persists */
#define UNET_TRACK_CLS_BOTH 3          /* present in both */
#define UNET_TRACK_CLS_GROWTH 4        /* b alone, inside a lesion that persists */
#define UNET_TRACK_CLS_NEW 5           /* a lesion of b alone that has no partner */
int32_t unet_vol_label_pairs(unet_ctx*, const int32_t* labels_a, int32_t n_a, const int32_t* labels_b, int32_t n_b, int32_t X, int32_t Y, int32_t Z, uint64_t* keys,
                             int64_t* counts, int64_t capacity, int64_t* info, void* stream);
int32_t unet_vol_track_map(unet_ctx*, const int32_t* labels_a, int32_t n_a, const int32_t* labels_b, int32_t n_b, int32_t X, int32_t Y, int32_t Z, const int32_t* lut_a,
                           const int32_t* lut_b, const uint8_t* cls_a, const uint8_t* cls_b, uint8_t* cls, int32_t* track_a, int32_t* track_b, int64_t* per_slice, void* stream);

/* ---- second-order texture of the CT under a mask (csrc/kernels_texture.hip; exact against tests/texture_oracle.py; texture.py) ----
 * All volumes: [X, Y, Z] in Fortran order, X Y Z < 2^31 (otherwise UNET_E_ARG, nothing launched).  Integer counts by integer atomics only: the same bits on every run.
 * All count outputs are int64, 8-byte aligned and OVERWRITTEN: the caller does not zero them.  A volume with a zero dimension returns UNET_OK with all counts zero.
 *
 * unet_vol_texture_quantize: vox / dtype / X, Y, Z / scaled, slope, inter, labels / mask / n / region: the volume, its decode and its groups exactly as for
 * unet_vol_intensity_bands (exactly one of labels and mask; a voxel takes part when its group lies in 1..n and region, when given, is non-zero there; a label outside 1..n
 * is ignored, never an address).  For a non-NaN value v, q = floor(fl(fl(v - lo) / width)), every operation rounded on its own.  outside = 0 (clip): the level is
 * min(max(q, 0), Ng - 1) + 1, so -inf is level 1 and +inf level Ng; outside = 1 (drop): the voxel takes no part when q < 0 or q >= Ng (the test is on q, not on v).  A NaN
 * value never takes part.  1 <= Ng <= UNET_VOL_TEXTURE_MAX_LEVELS, lo finite, width finite and > 0, outside 0 or 1: anything else is UNET_E_ARG and nothing is launched.
 *   levels        device uint8 [X Y Z]: 0 = takes no part, 1..Ng the level.  It alone says whether a voxel takes part: the two counting entries read it and `labels`.
 *   level_counts  device int64 [n][Ng]: the voxels of group g + 1 at every level (the first-order histogram on the same bins)
 *
 * unet_vol_texture_glcm / unet_vol_texture_runs: levels as written above (a level above Ng takes no part), labels int32 or null (null: every taking-part voxel is group 1,
 * the mask case); a label outside 1..n takes no part.  The 13 directions, in this fixed order, are bits 0..12 of `directions`:
 *   (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,-1,0) (1,0,1) (1,0,-1) (0,1,1) (0,1,-1) (1,1,1) (1,1,-1) (1,-1,1) (1,-1,-1)
 * directions = 0 or a bit above bit 12, Ng outside 1..UNET_VOL_TEXTURE_MAX_LEVELS, n < 0: UNET_E_ARG.
 *   glcm: counts[g - 1][k][a - 1][b - 1] += 1 for every selected direction k, every voxel p and q = p + distance dir_k inside the volume with levels[p] = a > 0,
 *   levels[q] = b > 0 and group(p) = group(q) = g.  Not symmetrised: the host forms C + C^T.  1 <= distance <= UNET_VOL_TEXTURE_MAX_DISTANCE.  merge != 0 sums all selected
 *   directions into one matrix (K = 1); otherwise K = popcount(directions), in ascending bit order.  counts: int64 [n][K][Ng][Ng].  While n K Ng^2 <=
 *   UNET_VOL_TEXTURE_LDS_COUNTERS a workgroup counts in an int32 table in LDS and leaves one 64-bit atomic per non-zero entry; beyond that every add is a 64-bit atomic.
 *   runs: along direction k with step 1 a run is a maximal sequence of consecutive voxels with one non-zero level a and one group g; counts[g - 1][k][a - 1][min(len,
 *   max_run) - 1] += 1 per run, and clamped[g - 1][k] += 1 when len > max_run (the last column then holds longer runs too: repeat with a larger max_run).
 *   1 <= max_run <= 2^15.  counts: int64 [n][K][Ng][max_run], clamped: int64 [n][K], K = popcount(directions). */
#define UNET_VOL_TEXTURE_MAX_LEVELS 64
#define UNET_VOL_TEXTURE_MAX_DISTANCE 4
#define UNET_VOL_TEXTURE_LDS_COUNTERS 8192
int32_t unet_vol_texture_quantize(unet_ctx*, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter,
                                  const int32_t* labels, const uint8_t* mask, int32_t n, const uint8_t* region, double lo, double width, int32_t Ng, int32_t outside,
                                  uint8_t* levels, int64_t* level_counts, void* stream);
int32_t unet_vol_texture_glcm(unet_ctx*, const uint8_t* levels, const int32_t* labels, int32_t n, int32_t X, int32_t Y, int32_t Z, int32_t Ng, int32_t distance,
                              int32_t directions, int32_t merge, int64_t* counts, void* stream);
int32_t unet_vol_texture_runs(unet_ctx*, const uint8_t* levels, const int32_t* labels, int32_t n, int32_t X, int32_t Y, int32_t Z, int32_t Ng, int32_t directions,
                              int32_t max_run, int64_t* counts, int64_t* clamped, void* stream);

/* ---- where the infection sits in the lungs (csrc/kernels_zones.hip; exact against tests/zones_oracle.py; zones.py) ----
 * All volumes: [X, Y, Z] in Fortran order, X Y Z < 2^31 (otherwise UNET_E_ARG, nothing launched); a volume with a zero dimension returns UNET_OK and touches nothing, the
 * outputs included.  Integer arithmetic only: a distance (the doubles unet_vol_edt_sq writes, 8-byte aligned) is compared as the order-preserving 64-bit key of its bit
 * pattern, key(u) = ~u when the sign bit is set, else u | 2^63 -- value order for non-negative values and +inf.  Sums are integers per wave (ballots) and per workgroup in
 * LDS, then 64-bit atomics; minima and maxima per lane, wave and workgroup, then one atomic: the same bits on every run.  All outputs are overwritten (the caller does not
 * initialise them).  sides: uint8 0 / 1 / 2, a value above 2 counts as 0.  A lane takes four voxels with one 4-byte load of sides when sides / infection / zone_map are
 * 4-byte and d2 / labels 16-byte aligned, one voxel otherwise.
 *
 * unet_vol_side_extents: box device int32 [2][6], per side value 1 and 2 the inclusive bounding box {x0, x1, y0, y1, z0, z1}; an empty side gives x0 = y0 = z0 = INT32_MAX
 * and x1 = y1 = z1 = -1.  dmax_key device uint64 [2]: with d2, the largest key of d2 under that side; 0 for an empty side or a null d2 (every key of a real distance is
 * above 0).  The host turns a key back into a double.
 *
 * unet_vol_zone_table: infection uint8, non-zero = infected, nullable; labels int32 with n lesions, nullable, a label outside 1..n is ignored, never an address; n < 0:
 * UNET_E_ARG; d2 nullable -- then every distance counts as +0.0, every voxel lies in shell 0 and spec->shells must be 1.  spec is a HOST pointer, read before the call
 * returns.  P = parts[0] parts[1] parts[2], S = shells, B = 2 P S <= UNET_VOL_ZONE_MAX_BINS.  For a voxel of side s (1 or 2) at coordinate c on axis a:
 *     d_a   = c - lo[s-1][a], or lo[s-1][a] + extent[s-1][a] - 1 - c when flip[a] (the coordinate counted from the other end of the range: the same voxels fall into
 *             the same part whichever way the axis is stored, also where the extent is no multiple of parts[a]);
 *     q_a   = clamp(floor(d_a parts[a] / extent[s-1][a]), 0, parts[a] - 1), in 64 bits;
 *     zone  = q_0 + parts[0] (q_1 + parts[1] q_2);      shell = #{k < S - 1 : key(d2) > key(r2[s-1][k])};      bin = ((s - 1) P + zone) S + shell.
 * UNET_E_ARG, nothing launched: parts outside 1..8, flip not 0 / 1, an extent < 1, shells outside 1..4, B above the maximum, r2[s][0 .. S-2] not finite, negative or
 * descending, a zone_map with 2 P > 255, a null or misaligned buffer.  Outputs (device, 8-byte aligned, int64 unless said otherwise):
 *   table           [B][2]   {lung voxels, infected voxels} of every bin
 *   outside         [1]      infected voxels under side 0
 *   lesion_zone     [n][2P]  the voxels of lesion i + 1 per (side, zone), in-lung voxels only            } may be null when n == 0
 *   lesion_shell    [n][S]   the same per shell                                                          }
 *   lesion_dmin_key [n]      uint64: the smallest key of d2 over the lesion's in-lung voxels, all ones when it has none   }
 *   zone_map        uint8 [X Y Z], nullable: 0 off the lungs, else 1 + (s - 1) P + zone
 * The bin table sits in LDS per workgroup and leaves once; the lanes of a wave that share a bin (a (lesion, bin) pair) are found with one ballot whose first lane adds the
 * popcount -- the per-lesion tables to LDS while n (2 P + S) <= 4096, straight to the outputs beyond that.  A wave with no lung voxel and no infected voxel reads neither
 * d2 nor the labels.  17 - 21 bytes read per voxel under the lungs, 1 - 2 elsewhere. */
#define UNET_VOL_ZONE_MAX_PARTS 8
#define UNET_VOL_ZONE_MAX_SHELLS 4
#define UNET_VOL_ZONE_MAX_BINS 1024
typedef struct unet_zone_spec {
  int32_t parts[3];        /* equal parts of the bounding range along every voxel axis, 1..8 */
  int32_t flip[3];         /* 1: the numbering runs against the axis */
  int32_t lo[2][3];        /* per side: the first coordinate of the divided range */
  int32_t extent[2][3];    /* per side: its length in voxels, >= 1 */
  int32_t shells;          /* S, 1..4 */
  int32_t reserved;        /* 0 */
  double r2[2][3];         /* per side: the squared radii between the shells, r2[s][0 .. S - 2] */
} unet_zone_spec;
int32_t unet_vol_side_extents(unet_ctx*, const uint8_t* sides, const double* d2, int32_t X, int32_t Y, int32_t Z, int32_t* box, uint64_t* dmax_key, void* stream);
int32_t unet_vol_zone_table(unet_ctx*, const uint8_t* sides, const uint8_t* infection, const int32_t* labels, int32_t n, const double* d2, int32_t X, int32_t Y, int32_t Z,
                            const unet_zone_spec* spec, int64_t* table, int64_t* outside, int64_t* lesion_zone, int64_t* lesion_shell, uint64_t* lesion_dmin_key,
                            uint8_t* zone_map, void* stream);

/* ---- rank filters of a CT: median, minimum, maximum, percentile, flat grey morphology (csrc/kernels_filter.hip; exact against
 * tests/filter_oracle.py and scipy.ndimage.rank_filter; filters.py) ----
 * src, dst: [X, Y, Z] in Fortran order, X Y Z < 2^31, the same element type and shape; they must not overlap.  dtype is the NIfTI code of the STORED element: 2 (uint8),
 * 256 (int8), 4 (int16), 512 (uint16), 8 (int32), 768 (uint32), 16 (float32); 64 is refused.  No slope or intercept enters: the filter orders stored elements.
 * Footprint: bit b = (dx + R) + (2 R + 1) ((dy + R) + (2 R + 1) (dz + R)) of the 128-bit word fp_hi:fp_lo says that the offset (dx, dy, dz), |d| <= R, belongs to it;
 * 1 <= R <= UNET_VOL_RANK_MAX_RADIUS, n = popcount in 1 .. (2 R + 1)^3, no bit at or above (2 R + 1)^3.
 * dst[v] = the element of rank `rank` (0 = the smallest, 0 <= rank < n) among src[v + o], o in the footprint: scipy.ndimage.rank_filter(a, rank, footprint=fp, mode=..)
 * with fp[dx + R, dy + R, dz + R].  Integers are ordered by value; float32 by the total order of the key bits ^ (sign ? 0xFFFFFFFF : 0x80000000): NaNs with the sign bit
 * set lowest, then -inf .. -0 < +0 .. +inf, the other NaNs highest.  The stored bits of the selected element are written unchanged; there is no float arithmetic.
 * Outside the volume, mode UNET_FILTER_NEAREST: the edge voxel repeats; UNET_FILTER_CONSTANT: the element whose stored bytes are the low bytes of cval_bits;
 * UNET_FILTER_REFLECT: scipy's default "reflect", index i reads p = i mod 2 n, and 2 n - 1 - p where p >= n (also for extents below R).
 * UNET_E_ARG, nothing launched, dst untouched: a null buffer or one not aligned to its element, src and dst overlapping, a bad dimension, dtype, R, footprint, rank or
 * mode, cval_bits with a bit above the element's width (in every mode).  A zero dimension touches nothing and returns UNET_OK.
 * One launch, no atomics, no workgroup waits for another: the same bits on every run. */
#define UNET_VOL_RANK_MAX_RADIUS 2
enum { UNET_FILTER_NEAREST = 0, UNET_FILTER_CONSTANT = 1, UNET_FILTER_REFLECT = 2 };
int32_t unet_vol_rank_filter(unet_ctx*, const void* src, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t R, uint64_t fp_lo, uint64_t fp_hi, int32_t rank,
                             int32_t mode, uint64_t cval_bits, void* dst, void* stream);

/* ---- a lung mask from the CT itself: the threshold pass and the growth from seeds inside a mask (csrc/kernels_lungmask.hip; exact against
 * tests/lungmask_oracle.py; lungs.py) ----
 * Volumes are [X, Y, Z] in Fortran order, X Y Z < 2^31.
 * unet_vol_threshold: vox, dtype, X, Y, Z, scaled, slope, inter as unet_vol_intensity_bands takes them (the eight NIfTI codes 2, 256, 4, 512, 8, 768, 16, 64).  The value
 *   of a voxel is v = double(raw), then (v * slope) + inter as two rounded operations when scaled: get_fdata's value.  mask[f] = 1 when lo <= v < hi and region is null or
 *   region[f] != 0, else 0; a NaN value gives 0.  lo = -inf and hi = +inf are allowed.  slice_counts (nullable): int64 [Z], overwritten with the set voxels of every slice.
 *   UNET_E_ARG, nothing launched, nothing written: a NaN edge or lo >= hi, NaN scaling, a bad dtype or dimension, a null or misaligned buffer (vox to its element,
 *   slice_counts to 8 bytes), mask overlapping vox or region.  A zero dimension touches nothing.  One launch over a bounded grid; the counts are integer sums.
 * unet_vol_geodesic_*: breadth-first growth of `seeds` inside `constraint` (uint8 volumes, set = non-zero).  By definition the result is the GEODESIC STEP DISTANCE
 *   inside the constraint: arrival[f] = the least number of steps of a path from a voxel of seeds & constraint to f that stays inside the constraint, each step moving to
 *   a neighbour under generate_binary_structure(3, connectivity) (planar: without its dz != 0 planes, connectivity 1 or 2; outside the volume is background); 0xFFFF
 *   where no such path exists or none of at most the steps run so far.  It is a count of steps, not millimetres.
 *   _ws_bytes  the workspace: four volumes of one bit per voxel in unet_vol_morph's packed layout (rows padded to 64-bit words): constraint, reached, two frontiers; 0 for
 *              a bad or zero dimension.
 *   _begin     packs constraint and seeds & constraint into the workspace, writes arrival (uint16 [X Y Z]: 0 on seeds & constraint, 0xFFFF elsewhere) and counts[0] =
 *              their number.  Seeds outside the constraint are ignored.
 *   _steps     runs the steps first_step .. first_step + n_steps - 1, one launch each: step s reaches the unreached constraint voxels that have a neighbour reached at
 *              step s - 1, stores s into their arrival and overwrites counts[s] (int64) with their number.  counts holds at least first_step + n_steps entries.  The calls
 *              after _begin continue each other: first_step is 1 after _begin and the previous call's last step + 1 afterwards, with the same X, Y, Z, connectivity, planar,
 *              arrival and workspace (the frontier of step s - 1 lives in the workspace).  After a step with counts[s] == 0 every later step finds nothing.  The host reads
 *              counts only between calls.
 *   Steps lie in 1 .. UNET_VOL_GEODESIC_MAX_STEP.  UNET_E_ARG, nothing launched: a bad dimension, connectivity, planar or step range, a null or misaligned buffer (arrival 2,
 *   counts 8, ws 16 bytes), a short workspace, arrival overlapping the workspace (or, in _begin, the seeds or the constraint).  A zero dimension touches nothing.
 *   No workgroup waits for another: a step boundary is a kernel boundary.  Integer work only: the same bits on every run. */
#define UNET_VOL_GEODESIC_MAX_STEP 65534
int32_t unet_vol_threshold(unet_ctx*, const void* vox, int32_t dtype, int32_t X, int32_t Y, int32_t Z, int32_t scaled, double slope, double inter, double lo, double hi,
                           const uint8_t* region, uint8_t* mask, int64_t* slice_counts, void* stream);
size_t unet_vol_geodesic_ws_bytes(int32_t X, int32_t Y, int32_t Z);
int32_t unet_vol_geodesic_begin(unet_ctx*, const uint8_t* seeds, const uint8_t* constraint, int32_t X, int32_t Y, int32_t Z, uint16_t* arrival, int64_t* counts, void* ws,
                                size_t ws_bytes, void* stream);
int32_t unet_vol_geodesic_steps(unet_ctx*, int32_t X, int32_t Y, int32_t Z, int32_t first_step, int32_t n_steps, int32_t connectivity, int32_t planar, uint16_t* arrival,
                                int64_t* counts, void* ws, size_t ws_bytes, void* stream);

/* ---- vesselness of a CT: Hessian eigenvalues and Frangi's tube measure (csrc/kernels_vessel.hip; exact against tests/vessel_oracle.py;
 * vessels.py) ----
 * L: a float32 volume [X, Y, Z] in Fortran order, X Y Z < 2^31, already smoothed at the scale sigma (millimetres) by unet_vol_smooth_axis.  Outside the volume the edge
 * voxel repeats (the Gaussian's only mode).  All arithmetic is float64, every operation rounded on its own (fl); the float32 samples convert exactly.
 * k: SIX HOST doubles, the scale-normalised (gamma = 1) factors computed once by the caller from sigma and the voxel size h:
 *   k[0..2] = kxx, kyy, kzz = sigma^2 / h_a^2;   k[3..5] = kxy, kxz, kyz = sigma^2 / (4 h_a h_b).
 * Hessian, 19 samples:  Hxx = fl(fl(fl(L[x+1] + L[x-1]) - fl(2 L[x])) kxx), likewise yy, zz;
 *   Hxy = fl(fl(fl(L[x+1,y+1] - L[x+1,y-1]) - fl(L[x-1,y+1] - L[x-1,y-1])) kxy), likewise xz, yz.
 * If any of the six entries is not finite, the three eigenvalues are the quiet NaN 0x7FC00000, the response is 0 and the voxel never becomes a best scale.
 * Eigenvalues: cyclic Jacobi on (a00, a11, a22, a01, a02, a12), pairs (0,1), (0,2), (1,2), five sweeps.  A rotation of (p, q), r the third index, is skipped when
 *   apq == 0 (so ending once all three off-diagonals are exactly 0 gives the same bits); otherwise theta = (aqq - app) / (2 apq), t = sgn(theta) / (|theta| +
 *   sqrt(theta^2 + 1)) with sgn(+-0) = +1, c = 1 / sqrt(t^2 + 1), s = t c, tau = s / (1 + c); app -= t apq, aqq += t apq; arp' = arp - s (arq + tau arp),
 *   arq' = arq + s (arp - tau arq), both from the old arp, arq; apq = 0.  An overflowing theta^2 needs no special case: IEEE gives sqrt = +inf and t = +-0.  The square
 *   root is the correctly rounded one, the division plain.
 * Order: the diagonal (a00, a11, a22) sorted by magnitude, |l1| <= |l2| <= |l3|, stable: exchange (1,2), (2,3), (1,2), each on strictly greater magnitude only.
 * Measure (Frangi): bright != 0 looks for tubes brighter than their surroundings, 0 for darker ones.  V = 0 unless l2 < 0 and l3 < 0 (dark: l2 > 0 and l3 > 0); else
 *   RA = |l2| / |l3|, RB = |l1| / sqrt(|l2| |l3|), S2 = (l1^2 + l2^2) + l3^2,
 *   V = float32(((1 - E(RA^2 / den_a)) E(RB^2 / den_b)) (1 - E(S2 / den_c))),   den_a = 2 alpha^2, den_b = 2 beta^2, den_c = 2 c^2 (from the host).
 * E(u) = exp(-u), the library's own: u = (u < 745 ? u : 745); k = rint(u INV_LN2); r = -((u - k LN2_HI) - k LN2_LO); p = the Taylor polynomial of degree 13 of e^r in
 *   Horner form, p = C13, p = p r + Cn for n = 12 .. 0, Cn = the double nearest 1 / n!; E = ldexp(p, -k).  INV_LN2 = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42fee00000p-1,
 *   LN2_LO = 0x1.a39ef35793c76p-33.
 * region (nullable, uint8 [X Y Z], non-zero = takes part): a voxel outside keeps eigenvalues +0.0, response 0, scale 0.
 * unet_vol_hessian_eig  writes eig = l1 | l2 | l3, three float32 volumes one after the other (3 X Y Z floats).
 * unet_vol_vesselness   reads and updates best (float32) and scale (uint8) in place for the scale of index `index`, 0 <= index < UNET_VOL_VESSEL_MAX_SCALES: index 0
 *   initialises them (best = V, scale = V > 0 ? 1 : 0); a later one replaces only where V > best, with scale = index + 1.  So over the scales of a call best is the maximum
 *   response and scale is 0 where best == 0, else 1 + the index of the first scale that reached the maximum.
 * UNET_E_ARG before any launch, nothing written: a null pointer (region aside), an extent <= 0 or X Y Z >= 2^31, a factor or denominator that is not finite and positive,
 *   bright outside 0 / 1, an index outside its range, a misaligned float buffer, an output overlapping L, the region or the other output.
 * One launch over a bounded grid of persistent workgroups, no atomics, every output element written by one lane: the same bits on every run. */
#define UNET_VOL_VESSEL_MAX_SCALES 254
int32_t unet_vol_hessian_eig(unet_ctx*, const float* L, int32_t X, int32_t Y, int32_t Z, const double* k, const uint8_t* region, float* eig, void* stream);
int32_t unet_vol_vesselness(unet_ctx*, const float* L, int32_t X, int32_t Y, int32_t Z, const double* k, const uint8_t* region, double den_a, double den_b, double den_c,
                            int32_t bright, int32_t index, float* best, uint8_t* scale, void* stream);

/* ---- centerlines of a mask volume: thinning, the table of a thin mask, label spread (csrc/kernels_skeleton.hip; exact against
 * tests/skeleton_oracle.py; skeleton.py) ----
 * Volumes are [X, Y, Z] in Fortran order, X Y Z < 2^31; set = non-zero; outside the volume is background; extents of 1 are legal (a 2-D image is Z = 1).
 * NEIGHBOUR MASK: the 26 neighbours of a voxel are numbered i = (dx + 1) + 3 (dy + 1) + 9 (dz + 1), i = 0 .. 26 without the centre 13; neighbour i is bit i (i < 13) or
 *   bit i - 1 (i > 13) of a uint32.  n26 = its popcount.
 * simple(v) (Bertrand and Malandain): the set neighbours form exactly one 26-connected component, and the clear voxels of the 18-neighbourhood that are 6-adjacent to v are
 *   not empty and lie in one 6-connected component of the clear voxels of the 18-neighbourhood.  25 985 144 of the 2^26 neighbourhoods are simple.
 * Thinning: an iteration is six direction passes +z, -z, +y, -y, +x, -x.  Pass d: the candidates, all judged on the image as the pass finds it, are the set voxels v with
 *   v + d clear or outside, n26(v) >= 2 (endpoints != 0) or >= 1 (endpoints == 0), and simple(v); then eight sub-passes k = 0 .. 7 clear, all at once, the candidates with
 *   (x & 1) | (y & 1) << 1 | (z & 1) << 2 == k that are still simple in the current image (only simplicity is tested again).  The result does not depend on the order lanes
 *   run in: two voxels of a subfield are never 26-neighbours.
 *   _ws_bytes     two volumes of one bit per voxel in unet_vol_morph's packed layout (rows padded to 64-bit words): the image and the candidates; 0 for a bad or zero
 *                 dimension.
 *   _begin        packs mask (bytes, any alignment) into the workspace.
 *   _iterations   runs the iterations first .. first + n - 1 (6 x 9 launches each) and overwrites removed[it] (int64, 8-byte aligned, at least first + n entries) with the
 *                 voxels iteration it cleared.  The host reads removed only between calls and stops after the first iteration that cleared nothing.
 *   _end          unpacks the image into out (bytes 0 / 1, any alignment).
 *   UNET_E_ARG, nothing launched: a bad dimension, first < 0, n < 0, endpoints outside 0 / 1, a null or misaligned buffer (removed 8, ws 16 bytes), a workspace below
 *   _ws_bytes, a buffer overlapping the workspace.  A zero dimension, or n == 0, launches nothing.
 * Table: the set voxels of a mask sorted by flat index, by count -> scan -> emit.
 *   unet_vol_skeleton_count   *total (device int64) = the set voxels; ws (unet_vol_skeleton_ws_bytes) keeps the offsets for _emit.
 *   unet_vol_skeleton_emit    the same mask and ws after the host has read the total and passes it back with the capacity of the outputs: index int32 [capacity] the flat
 *                             index, nbr uint32 [capacity] the neighbour mask, and, when d2 (float64 [X Y Z], e.g. of unet_vol_edt_sq) and vals (float64 [capacity]) are
 *                             both given, vals[i] = d2[index[i]].  capacity < total is UNET_E_ARG; no row at or past capacity is ever written.
 *   UNET_E_ARG, nothing launched: a bad dimension, a null or misaligned buffer (index, nbr 4, d2, vals, total 8, ws 16 bytes), a short workspace, total or capacity out of
 *   range, only one of d2 / vals, an output overlapping an input or another output.
 * unet_vol_label_spread: arrival is what unet_vol_geodesic_* wrote (uint16), labels int32 [X Y Z], non-zero on the voxels of arrival 0 that carry a label.  One launch per
 *   step s = first .. first + n - 1: a voxel with arrival == s takes the smallest non-zero label among its neighbours under generate_binary_structure(3, connectivity) whose
 *   arrival == s - 1, and keeps its label when there is none.  A launch writes only step-s voxels and reads only step-(s - 1) voxels.  UNET_E_ARG, nothing launched: a bad
 *   dimension or connectivity, first < 1, n < 0, a step beyond UNET_VOL_GEODESIC_MAX_STEP, a null or misaligned buffer, labels overlapping arrival.
 * Integer work only, no workgroup waits for another, every grid is sized to its work: the same bits on every run. */
size_t unet_vol_thin_ws_bytes(int32_t X, int32_t Y, int32_t Z);
int32_t unet_vol_thin_begin(unet_ctx*, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, void* ws, size_t ws_bytes, void* stream);
int32_t unet_vol_thin_iterations(unet_ctx*, int32_t X, int32_t Y, int32_t Z, int32_t first, int32_t n, int32_t endpoints, int64_t* removed, void* ws, size_t ws_bytes,
                                 void* stream);
int32_t unet_vol_thin_end(unet_ctx*, int32_t X, int32_t Y, int32_t Z, uint8_t* out, const void* ws, size_t ws_bytes, void* stream);
size_t unet_vol_skeleton_ws_bytes(int32_t X, int32_t Y, int32_t Z);
int32_t unet_vol_skeleton_count(unet_ctx*, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int64_t* total, void* ws, size_t ws_bytes, void* stream);
int32_t unet_vol_skeleton_emit(unet_ctx*, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, const double* d2, int64_t total, int64_t capacity, int32_t* index,
                               uint32_t* nbr, double* vals, const void* ws, size_t ws_bytes, void* stream);
int32_t unet_vol_label_spread(unet_ctx*, const uint16_t* arrival, int32_t* labels, int32_t X, int32_t Y, int32_t Z, int32_t first, int32_t n, int32_t connectivity,
                              void* stream);

/* ---- marker-controlled watershed and cost-weighted geodesic distance on a volume, the depth cost (csrc/kernels_watershed.hip; exact against
 * tests/watershed_oracle.py; watershed.py) ----
 * Volumes are [X, Y, Z] in Fortran order, X Y Z < 2^31; outside the volume there is nothing; extents of 1 are legal.
 * cost uint32 per voxel.  markers int32 per voxel: 1 .. 2^24 - 1 a marker, 0 none, anything else is invalid -- counted, treated as none, never an address.  mask: bytes,
 * or null for "everywhere"; a voxel where it is zero takes no part, a marker there is ignored.  Neighbours: generate_binary_structure(3, connectivity), 1, 2 or 3.
 * Each phase is the greatest fixed point, below "unreached", of a monotone operator, so the result is unique and independent of the order of updates:
 *   HEIGHT  the pass height H: H[v] = cost[v] on a marker, elsewhere min over neighbours n of max(H[n], cost[v]); 0xFFFFFFFF where no marker is connected in the mask.
 *   LABEL   on the finished H: an edge n -> v is tight when max(H[n], cost[v]) == H[v]; key = steps << 32 | label; a marker holds (0, its label), every other voxel the
 *           minimum over its tight neighbours of key[n] + (1 << 32).  A voxel goes to the marker nearest in steps along pass-height-realising paths, among equally near
 *           markers to the lowest label; a plateau is divided by step distance.  Every voxel with a finite H receives a label.
 *   SUM     key = dist << 24 | label, dist 40 bits; a marker holds (0, label), elsewhere the minimum over neighbours of (dist[n] + cost[v], label[n]); a candidate whose
 *           distance would exceed 2^40 - 2 is no candidate.  A mask voxel that ends unreached beside a reached neighbour is counted as overflowed.
 * The watershed (rule "max") is HEIGHT to its fixed point, then LABEL to its fixed point; the label is not carried in the height key because height << k | label is not
 * monotone ((3, 2) < (4, 1), but through a voxel of cost 5: (5, 2) > (5, 1)).
 *   _ws_bytes   two buffers of a 64-bit key per voxel, the heights, per-brick bytes and partial counts; 0 for a bad or zero dimension.
 *   _begin      seeds both key buffers for `phase` and notes the invalid markers.  LABEL: first keeps the heights of the HEIGHT phase, `done` = the HEIGHT sweeps that were
 *               run (it says which buffer holds them); other phases ignore done (>= 0).
 *   _sweeps     runs the sweeps first .. first + n - 1 of `phase` (one launch each: sweep s reads key buffer s & 1 and writes the other) and overwrites changed[s] (int64,
 *               8-byte aligned, at least first + n entries) with the voxels whose key sweep s lowered.  The host reads changed only between calls and stops after the first
 *               sweep with changed == 0: the state is then the fixed point.  skip = 1: a 32 x 8 x 8 brick whose own and 26 neighbour bricks' keys the previous sweep left
 *               alone is not visited; skip = 0 visits every brick with a mask voxel; the results, changed included, are the same.
 *   _end        `done` = the sweeps of `phase` that were run.  HEIGHT: height.  LABEL: labels (int32, 0 unreached), steps (uint32, 0xFFFFFFFF unreached) and, when not
 *               null, height.  SUM: labels and distance (uint64, 2^40 - 1 unreached).  Outputs the phase does not write must be null.  counts (int64 [4], 8-byte
 *               aligned): voxels reached, mask voxels unreached, overflowed (SUM; else 0), invalid markers.  A zero dimension: counts = 0.
 *   UNET_E_ARG, nothing launched, nothing written: a bad dimension, connectivity or phase, first < 0, n < 0, done < 0, skip outside 0 / 1, a null or misaligned buffer
 *   (cost, markers, labels, height, steps 4, changed, distance, counts 8, ws 16 bytes), a workspace below _ws_bytes, an input or output overlapping the workspace, an
 *   output overlapping the mask or another output.  A zero dimension, or n == 0, launches nothing.
 * Every sweep, every changed[s] and the sweep count are the same on every run: a launch reads what earlier launches wrote and every element is written by one lane.  Integer
 * arithmetic, no atomics but changed[s], no workgroup waits for another; a sweep's grid is bounded (at most 2048 workgroups walk the bricks).
 * unet_vol_depth_cost: cost[v] = uint32(floor((d2max - d2[v]) / quantum)) in float64, every operation rounded on its own, clipped to 0 .. 2^32 - 2; 0 where mask (bytes, or
 *   null) is zero.  UNET_E_ARG: a bad dimension, quantum not positive and finite, d2max negative or not finite, a null or misaligned buffer, cost overlapping an input. */
#define UNET_VOL_WATERSHED_HEIGHT 0
#define UNET_VOL_WATERSHED_LABEL 1
#define UNET_VOL_WATERSHED_SUM 2
size_t unet_vol_watershed_ws_bytes(int32_t X, int32_t Y, int32_t Z);
int32_t unet_vol_watershed_begin(unet_ctx*, const uint32_t* cost, const int32_t* markers, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t phase, int32_t done,
                                 void* ws, size_t ws_bytes, void* stream);
int32_t unet_vol_watershed_sweeps(unet_ctx*, const uint32_t* cost, const int32_t* markers, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t first, int32_t n,
                                  int32_t phase, int32_t connectivity, int32_t skip, int64_t* changed, void* ws, size_t ws_bytes, void* stream);
int32_t unet_vol_watershed_end(unet_ctx*, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, int32_t phase, int32_t done, int32_t connectivity, int32_t* labels,
                               uint32_t* height, uint32_t* steps, uint64_t* distance, int64_t* counts, const void* ws, size_t ws_bytes, void* stream);
int32_t unet_vol_depth_cost(unet_ctx*, const double* d2, const uint8_t* mask, int32_t X, int32_t Y, int32_t Z, double d2max, double quantum, uint32_t* cost, void* stream);

/* ------------------------------------------------------------------------------------
 * Model level. Replaces the Keras Model built at T1:853-916 and driven by
 * compile/fit/evaluate/predict (T1:1053-1061, 1101, 1137).  A model is a fixed-shape plan:
 * three op programs (training forward, backward, inference forward) over caller-owned
 * flat buffers.  Programs can be run in [begin,end) slices so a data-parallel host can put
 * collectives between ops (sync points) and overlap gradient all-reduce with backward.
 * ---------------------------------------------------------------------------------- */
enum { UNET_PROG_FWD_TRAIN = 0, UNET_PROG_BWD = 1, UNET_PROG_FWD_INFER = 2 };

typedef struct unet_sync_point {
  int32_t after_op;   /* run ops [.., after_op] then reduce */
  int32_t kind;       /* 0 = bn fwd sums, 1 = loss sums, 2 = bn bwd sums, 3 = grad bucket ready */
  void* ptr;          /* device pointer of the doubles (kinds 0-2) / floats (kind 3) to SUM-reduce */
  int64_t count;      /* number of elements */
  int32_t use_op;     /* kinds 0-2: the first op that READS the reduced values (> after_op).  use_op > after_op + 1 means the ops in between do not depend on
                         the reduction: the host may run it on a side stream beside them and make the compute stream wait just before use_op (the backward
                         programs place an independent weight gradient there).  Kind 3: the number of ops of the program (the optimizer is the reader). */
  int32_t reserved;
} unet_sync_point;

/* The SUM all-reduce of a sync point of kinds 0-2, device side (data parallelism is new: the reference is single-process, T1:1053-1061 runs one
 * model.fit).  Every rank of ONE node owns a receive area in fine-grained HBM that its peers map through HIP IPC; one kernel on `stream` pushes the rank's
 * doubles into every peer's area (xGMI is point to point: the W - 1 copies travel on W - 1 links at once), polls its own area until all W contributions of
 * this call have landed and adds them in rank order -- every rank ends with the same bits.  No host proxy, no ring: one fabric latency per reduction.
 *   unet_comm_create   allocates the area and returns its 64-byte IPC handle in handle_out; the host exchanges the handles of all ranks by any means it has
 *                      (torch.distributed.all_gather_object in engine.py) and passes them, in rank order, to
 *   unet_comm_connect  (handles = world x UNET_COMM_HANDLE_BYTES bytes; the own entry is ignored).
 *   unet_comm_allreduce_f64  buf[0..count) <- sum over ranks, in place (one launch per UNET_COMM_MAX_DOUBLES).  Every rank must issue the same calls in the same order.
 *                      A contribution that does not arrive within the timeout (default 60 s) ends the kernel and latches the communicator's error word:
 *   unet_comm_status   *err_out = 0, or 1 + the rank that was missing (sticky; the reduced values of that call are not valid).  Synchronises `stream`.
 * Gradient buckets (kind 3) are bandwidth-bound and stay with RCCL.  A rank may destroy its communicator once its own last all-reduce has completed (by then every
 * peer has written all it will ever write into this rank's area). */
#define UNET_COMM_HANDLE_BYTES 64
#define UNET_COMM_MAX_WORLD 8
#define UNET_COMM_MAX_DOUBLES 2048
typedef struct unet_comm unet_comm;
int32_t unet_comm_create(unet_ctx*, int32_t rank, int32_t world, unet_comm** out, unsigned char* handle_out);
int32_t unet_comm_connect(unet_comm*, const unsigned char* handles);
int32_t unet_comm_set_timeout_ms(unet_comm*, int32_t ms);
int32_t unet_comm_allreduce_f64(unet_comm*, double* buf, int32_t count, void* stream);
int32_t unet_comm_status(unet_comm*, int32_t* err_out, void* stream);
void unet_comm_destroy(unet_comm*);

/* arch: UNET_ARCH_UNET (T1:853-916), UNET_ARCH_UNETPP (task1_unet_plus_plus.py:858-950) or UNET_ARCH_CLASSIFIER (the Sequential
 * CNN of task2_covid19_classifcation.py:747-776: y_true / p_out are [n] floats, loss_ptr = (binary cross-entropy, f1)) */
enum { UNET_ARCH_UNET = 0, UNET_ARCH_UNETPP = 1, UNET_ARCH_CLASSIFIER = 2 };
/* dtype: UNET_DTYPE_F32, or UNET_DTYPE_BF16 = activations / activation gradients stored as bf16 inside the workspace (the image x,
 * the targets, the probabilities p_out, parameters, gradients and optimizer state stay fp32; in_ch must be 1) */
int32_t unet_model_create(unet_ctx*, int32_t arch, int32_t in_ch, int32_t n, int32_t h, int32_t w,
                          int32_t world_size, int32_t conv_algo, int32_t dtype, unet_model** out);
int32_t unet_model_dtype(const unet_model*);
void unet_model_destroy(unet_model*);
int64_t unet_model_param_count(const unet_model*);   /* trainable floats (7,762,401 for in_ch=1) */
int64_t unet_model_state_count(const unet_model*);   /* BN moving mean/var floats (2,880) */
size_t unet_model_workspace_bytes(const unet_model*, int32_t training);
/* offsets (in floats) of a named tensor inside the flat param / state buffers; name as in
 * Keras order: "c1a/kernel", "bn1/gamma", "bn1/mean", "u6/kernel", "out/bias", ... */
int32_t unet_model_tensor_info(const unet_model*, const char* name, int32_t* is_state,
                               int64_t* offset, int64_t* count);
int32_t unet_model_bind(unet_model*, float* params, float* grads, float* adam_m, float* adam_v,
                        float* bn_state, void* workspace, size_t workspace_bytes);
int32_t unet_model_set_io(unet_model*, const float* x, const float* y_true, float* p_out);
/* loss_out: device float[2] of the caller's that the next forward programs ALSO write (loss, metric) to -- a training loop that collects one pair per step
 * (model.fit reads them once per epoch, T1:1059) hands in a fresh slot per step instead of copying unet_model_loss_ptr behind every step; NULL = none (ABI v15) */
int32_t unet_model_set_loss_out(unet_model*, float* loss_out);
int32_t unet_model_set_dropout(unet_model*, float rate, uint64_t seed);
/* classifier only: weights of class 0 / class 1 in the loss (Keras class_weight, T2:835); default 1, 1 */
int32_t unet_model_set_class_weights(unet_model*, float w0, float w1);
/* U-Net / U-Net++: the training loss (UNET_LOSS_*; alpha, beta > 0: Tversky's weights, ignored by the others); default UNET_LOSS_BCE_DICE.  Valid between runs
 * of a built model (Keras compiles after it builds the graph, and may compile again, T1:1208): the programs read it when they run.  The weighted loss adds the
 * weight-map op to the forward programs, n h w floats to the workspace (unet_model_workspace_bytes reflects the loss that is set; a bound workspace that is too
 * small for it: UNET_E_STATE, nothing changed) and a fifth double to the loss-sum sync point (unet_model_sync_points: re-read after this call).  The classifier
 * keeps binary cross-entropy: any other loss is UNET_E_ARG there. */
int32_t unet_model_set_loss(unet_model*, int32_t loss, float alpha, float beta);
int32_t unet_model_num_ops(const unet_model*, int32_t prog);
int32_t unet_model_sync_points(const unet_model*, int32_t prog, unet_sync_point* out, int32_t cap);
int32_t unet_model_run(unet_model*, int32_t prog, int32_t begin, int32_t end, void* stream);
/* device pointer to float[2] = (loss, dice_coeff) of the last forward with y_true bound */
const float* unet_model_loss_ptr(const unet_model*);
/* intermediate activation / gradient taps for tests ("c1a","bn1","p1","u6","cat6",...) */
int32_t unet_model_tap(const unet_model*, const char* name, int32_t grad, const void** ptr,   /* element size: unet_model_tap_elem_bytes */
                       int32_t* ld, int32_t* n, int32_t* h, int32_t* w, int32_t* c);
int32_t unet_model_tap_elem_bytes(const unet_model*, const char* name, int32_t grad);   /* 4 (float) or 2 (unet_bf16) */
/* profiling: per-op name and accumulated milliseconds since last reset (profiling on) */
int32_t unet_model_op_info(const unet_model*, int32_t prog, int32_t op, const char** name,
                           double* flops, double* bytes, double* ms, int64_t* calls);
int32_t unet_model_reset_timers(unet_model*);

#ifdef __cplusplus
}
#endif
#endif /* UNET_HIP_H */
