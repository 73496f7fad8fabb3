/*
 * sqdet.h -- C ABI of libsqdet_hip.so: the MI355X (gfx950) SqueezeDet hot path.
 *
 * The reference (BichenWuUCB/squeezeDet, TF 1.0 / Python 2.7) has NO FFI or
 * operator-plugin interface: its boundary is Python-level -- builder methods on
 * ModelSkeleton plus the model-object contract used by demo.py/eval.py/train.py
 * (SURVEY.md 8b).  This header is the C-ABI a maintainer would bind in place of
 * the TF graph ops those builders emit; every entry point cites the reference
 * interface it replaces (paths relative to the reference's src/).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / HIP C++ types.
 *   - every data pointer is a CALLER-OWNED DEVICE pointer unless the name says
 *     "host"; nothing here allocates device memory.
 *   - sqdet_stream_t is a hipStream_t passed as void* (NULL = default stream);
 *     calls enqueue work on that stream and return without synchronising.
 *   - return value: SQDET_OK (0) or a negative SQDET_E* code; never throws.
 *     sqdet_last_error() returns a thread-local message for the last failure.
 *   - activations are NHWC; conv kernels are HWIO [kh,kw,Cin,Cout] float32
 *     (the reference's '<layer>/kernels' variables, nn_skeleton.py:531-533) and
 *     are re-laid-out once into MFMA fragment order by sqdet_conv_pack_weights.
 *   - dtype is the STORAGE type of activations/weights (SQDET_F16 or SQDET_F32);
 *     accumulation is always float32; biases are always float32.
 */
#ifndef SQDET_H
#define SQDET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sqdet_stream_t;

enum { SQDET_OK = 0, SQDET_EINVAL = -1, SQDET_EUNSUPPORTED = -2, SQDET_EHIP = -3, SQDET_ESTATE = -4 };
enum { SQDET_F32 = 0, SQDET_F16 = 1 };
enum { SQDET_PAD_SAME = 0, SQDET_PAD_VALID = 1 };
enum { SQDET_ARCH_SQUEEZEDET = 0, SQDET_ARCH_SQUEEZEDET_PLUS = 1, SQDET_ARCH_RESNET50 = 2, SQDET_ARCH_VGG16 = 3 };

const char* sqdet_version(void);
const char* sqdet_last_error(void);
/* Tuning knobs (process-wide).  "conv_algo": 0 = auto (specialised kernels when eligible,
 * default), 1 = generic implicit-GEMM kernels only (also env SQDET_CONV_ALGO=generic).
 * "fire_fuse": 0 = plan heuristic (default), 1 = one launch per fire module wherever the kernels cover it, 2 = never
 * fuse, 3 = no streaming kernel, 4 = fire modules and the pools behind them stay apart, 5 = no fire-module chains, 6 = chains on
 * the late (small) maps only, 7 = a run's first module as squeeze conv + chain launch instead of one streaming launch,
 * 8 = no streaming expand + next-squeeze launches (a pooled module then ends its run).
 * "stem_algo": which kernel runs the fused conv1 + pool1 launch: 0 = the fastest that takes the shape (default), 2 = the strip
 * kernel only (no stem + squeeze launch), 3 = the persistent strip-lane kernel, then the strip kernel (propagates NaN / Inf pixels
 * like conv -> pool).  Any other value: SQDET_EINVAL, the option keeps its value.
 * "conv_pool": 1 = a 3x3 conv and the 2x2/s2 SAME max-pool behind it are one launch wherever the tile kernel takes the shape
 * (default), 0 = never (plans created afterwards and sqdet_conv2d_maxpool2_*). */
int sqdet_set_option(const char* name, int value);

/* ------------------------------------------------------------------ conv --
 * Replaces ModelSkeleton._conv_layer (nn_skeleton.py:471-563):
 *   relu?(conv2d(x, W, [1,s,s,1], padding) + b), TF SAME/VALID semantics
 *   (asymmetric SAME: the extra pad cell goes bottom/right).
 */

/* Bytes of the packed (MFMA fragment order) form of a [k,k,cin,cout] kernel. */
size_t sqdet_conv_packed_bytes(int k, int cin, int cout, int dtype);

/* w_hwio_f32: device float32 [k,k,cin,cout] -> packed (dtype storage). */
int sqdet_conv_pack_weights(const float* w_hwio_f32, void* packed, int k, int cin, int cout, int dtype,
                            sqdet_stream_t stream);

/* x: [n,h,w,cin] -> y: [n,ho,wo,*] written at channel offset y_coffset of rows
 * y_cstride channels wide (y_cstride=cout, y_coffset=0 for a plain conv; a fire
 * module's two expand convs write the two halves of one concat tensor,
 * nets/squeezeDet.py:106).  bias: float32 [cout].  relu: 0/1. */
int sqdet_conv2d_nhwc_fwd(const void* x, const void* w_packed, const float* bias, void* y,
                          int n, int h, int w, int cin, int cout, int k, int stride, int pad_mode, int relu,
                          int dtype, int y_cstride, int y_coffset, sqdet_stream_t stream);

/* The ConvDet head (nets/squeezeDet.py:76-79: conv12, 3x3 / SAME, no ReLU) TOGETHER WITH the score half of
 * _add_interpretation_graph (nn_skeleton.py:150-170, 274-283): preds [n,h,w,apg*(classes+5)] as sqdet_conv2d_nhwc_fwd would
 * write them, and scores float32 [n, h*w*apg] = det_probs (max over classes of softmax(class logits) * sigmoid(confidence)),
 * computed in the conv's epilogue from the float16-rounded preds with the float expressions of sqdet_interpret_output --
 * bitwise the det_probs that call returns.  float16, anchors_per_grid 9, classes 3, Cin a multiple of 128 (the split-K
 * ConvDet kernel); SQDET_EUNSUPPORTED otherwise (sqdet_convdet_scores_supported tells in advance).  Follow with
 * sqdet_detect_filter_scored: the whole post-processing is then one 32-workgroup launch. */
int sqdet_convdet_fwd(const void* x, const void* w_packed, const float* bias, void* preds, float* scores, int n, int h, int w,
                      int cin, int anchors_per_grid, int classes, int dtype, sqdet_stream_t stream);
int sqdet_convdet_scores_supported(int cin, int anchors_per_grid, int classes, int dtype);

/* Residual form used by ResNet50ConvDet (nets/resnet50_convDet.py:55, `tf.nn.relu(branch1+branch2)`):
 *   y = relu?(conv2d(x, W) + b + y)   -- y holds the shortcut branch on entry, the block output on exit
 * (the branch2c 1x1 conv of a bottleneck adds its result to the shortcut in its own epilogue, so
 * the sum never makes an extra HBM round trip).  Same arguments as sqdet_conv2d_nhwc_fwd. */
int sqdet_conv2d_add_nhwc_fwd(const void* x, const void* w_packed, const float* bias, void* y_inout,
                              int n, int h, int w, int cin, int cout, int k, int stride, int pad_mode, int relu,
                              int dtype, int y_cstride, int y_coffset, sqdet_stream_t stream);
/* The same with the shortcut in a tensor of its own (rows of y_cstride channels, like y), left untouched:
 *   y = relu?(conv2d(x, W) + b + residual)
 * -- the training forward keeps every block input for the backward pass (nn_skeleton.py:329-361 differentiates through
 * resnet50_convDet.py:55), so the sum must not overwrite the shortcut.  Only channels [y_coffset, y_coffset+cout) of y are
 * written, and only the same channels of residual are read; the rest of both rows stays as it was.  1x1 convs read the
 * residual tile in their epilogue (conv1x1_pipe); other shapes copy that channel slice into y first. */
int sqdet_conv2d_res_nhwc_fwd(const void* x, const void* w_packed, const float* bias, const void* residual, void* y,
                              int n, int h, int w, int cin, int cout, int k, int stride, int pad_mode, int relu,
                              int dtype, int y_cstride, int y_coffset, sqdet_stream_t stream);

/* ------------------------------------------------------------- batch norm --
 * Replaces the frozen-statistics batch norm of ModelSkeleton._conv_bn_layer (nn_skeleton.py:374-468:
 * tf.nn.batch_normalization(conv [+ biases], mean, var, offset=beta, scale=gamma, eps) with mean/var
 * non-trainable constants) by folding it into the conv it follows:
 *   inv = gamma / sqrt(var + eps);  w_folded[..., c] = w[..., c] * inv[c];
 *   b_folded[c] = (conv_bias[c] - mean[c]) * inv[c] + beta[c]          (conv_bias may be NULL = 0)
 * w_hwio / w_folded: float32 [k,k,cin,cout] (may alias); the per-channel vectors float32 [cout]. */
int sqdet_fold_batchnorm(const float* w_hwio, const float* conv_bias, const float* gamma, const float* beta,
                         const float* mean, const float* var, float eps, float* w_folded, float* b_folded,
                         int k, int cin, int cout, sqdet_stream_t stream);

/* Training of a _conv_bn_layer conv (the trainable res4* blocks, resnet50_convDet.py:94-118): the conv
 * backward kernels produce the gradients of the FOLDED kernel / bias; this turns them into the
 * gradients of the variables (float32):  dw = dw_folded * gamma/sqrt(var+eps)  (may alias dw_folded),
 *   dgamma = (sum over k,k,cin of dw_folded * w + (conv_bias - mean) * db_folded) / sqrt(var+eps),
 *   dbeta = db_folded.   conv_bias may be NULL.  workspace: sqdet_fold_batchnorm_bwd_workspace_bytes(...) of device
 *   scratch (per-row-block column sums, added in a fixed order: deterministic). */
size_t sqdet_fold_batchnorm_bwd_workspace_bytes(int k, int cin, int cout);
int sqdet_fold_batchnorm_bwd(const float* w_hwio, const float* dw_folded, const float* db_folded,
                             const float* conv_bias, const float* gamma, const float* mean, const float* var, float eps,
                             float* dw, float* dgamma, float* dbeta, float* workspace, int k, int cin, int cout,
                             sqdet_stream_t stream);
/* The same for MANY convs in two launches (per conv the results are bitwise sqdet_fold_batchnorm_bwd's: its kernels' own
 * device code, run on a workgroup range per conv -- the table mechanism of sqdet_conv_pack_many and sqdet_slab_reduce_many): prepare() fills
 * a host table of sqdet_fold_batchnorm_bwd_many_table_bytes(n_items) bytes from per-item pointer arrays (conv_bias[i] may
 * be NULL; workspace[i]: that conv's sqdet_fold_batchnorm_bwd_workspace_bytes) and reports the two grids; the caller copies
 * the table to the device once. */
size_t sqdet_fold_batchnorm_bwd_many_table_bytes(int n_items);
int sqdet_fold_batchnorm_bwd_many_prepare(const float* const* w_hwio, const float* const* dw_folded,
                                          const float* const* db_folded, const float* const* conv_bias,
                                          const float* const* gamma, const float* const* mean, const float* const* var,
                                          float* const* dw, float* const* dgamma, float* const* dbeta, float* const* workspace,
                                          const int* k, const int* cin, const int* cout, int n_items, void* table_host,
                                          int* blocks, int* finish_blocks);
int sqdet_fold_batchnorm_bwd_many(const void* table_dev, int n_items, int blocks, int finish_blocks, float eps,
                                  sqdet_stream_t stream);

/* y[n,oy,ox,:] = x[n,oy*stride,ox*stride,:], y: [n,ceil(h/stride),ceil(w/stride),c] -- the pixels a 1x1
 * stride-s SAME conv reads (res3a/res4a branch1 and branch2a), so that their filter gradient can use
 * sqdet_conv2d_nhwc_bwd_filter (stride 1) on the gathered tensor. */
int sqdet_subsample_nhwc(const void* x, void* y, int n, int h, int w, int c, int stride, int dtype,
                         sqdet_stream_t stream);

/* ------------------------------------------------------------------ pool --
 * Replaces ModelSkeleton._pooling_layer (nn_skeleton.py:565-586): tf.nn.max_pool,
 * SAME-padded cells never win.  x: [n,h,w,c] -> y: [n,ho,wo,c]. */
int sqdet_maxpool_nhwc_fwd(const void* x, void* y, int n, int h, int w, int c, int k, int stride, int pad_mode,
                           int dtype, sqdet_stream_t stream);
/* The training forward's pool (k = 3, any stride, or k = 2, stride 2): also records, per output element, which window cell
 * won -- one byte, k * row + column of the FIRST maximum in row-major order (tf.nn.max_pool's gradient convention); a window
 * that nothing wins (all -inf / NaN) names its first valid cell -- for sqdet_maxpool_nhwc_bwd_idx.  window_index: [n,ho,wo,c]
 * uint8.  y is bitwise sqdet_maxpool_nhwc_fwd's. */
int sqdet_maxpool_nhwc_fwd_idx(const void* x, void* y, unsigned char* window_index, int n, int h, int w, int c, int k,
                               int stride, int pad_mode, int dtype, sqdet_stream_t stream);

/* conv 3x3/s1/SAME (+ ReLU when relu = 1) followed by max_pool 2x2/s2/SAME in ONE launch (VGG16's conv1_2+pool1 .. conv4_3+pool4,
 * nets/vgg16_convDet.py:40-78): the conv's full-resolution output never reaches HBM.  x: [n,h,w,cin]; w_packed: packed 3x3 kernel;
 * bias: float32 [cout] (required); y: [n,ceil(h/2),ceil(w/2),cout].  Bitwise sqdet_conv2d_nhwc_fwd followed by
 * sqdet_maxpool_nhwc_fwd(k 2, stride 2, SAME).  SQDET_EUNSUPPORTED where sqdet_conv2d_maxpool2_supported says 0 (among others:
 * Cin not a multiple of 8 halves / 4 floats, Cout not a multiple of 4, conv_algo = generic, option "conv_pool" = 0). */
int sqdet_conv2d_maxpool2_nhwc_fwd(const void* x, const void* w_packed, const float* bias, void* y, int n, int h, int w,
                                   int cin, int cout, int relu, int dtype, sqdet_stream_t stream);
/* 1 if sqdet_conv2d_maxpool2_nhwc_fwd takes the shape, else 0 (callers branch instead of catching SQDET_EUNSUPPORTED).  The same
 * answer holds for sqdet_conv2d_maxpool2_nhwc_fwd_idx. */
int sqdet_conv2d_maxpool2_supported(int n, int h, int w, int cin, int cout, int dtype);
/* sqdet_conv2d_maxpool2_nhwc_fwd that also writes the pool's window index [n,ceil(h/2),ceil(w/2),cout] uint8 (the training forward
 * of VGG16's conv3_3+pool3 and conv4_3+pool4): y bitwise sqdet_conv2d_maxpool2_nhwc_fwd's, window_index bitwise
 * sqdet_maxpool_nhwc_fwd_idx(k 2, stride 2, SAME) of the unfused conv's stored output. */
int sqdet_conv2d_maxpool2_nhwc_fwd_idx(const void* x, const void* w_packed, const float* bias, void* y, unsigned char* window_index,
                                       int n, int h, int w, int cin, int cout, int relu, int dtype, sqdet_stream_t stream);

/* ------------------------------------------------------------------ stem --
 * conv1 + pool1 in one launch: relu(conv2d(x, W, stride 2) + b) followed by max_pool 3x3/s2
 * (nets/squeezeDet.py:40-44: k=3, 64 filters, SAME/SAME; nets/squeezeDetPlus.py:40-44: k=7,
 * 96 filters, VALID/VALID).  x: [n,h,w,3]; y: [n,hp,wp,cout].  Only those two stems are fused.
 * Like sqdet_conv2d_nhwc_fwd, both stem calls refuse a NULL operand and non-positive n / h / w / cout / k (/ next_s) with
 * SQDET_EINVAL before anything is launched. */
int sqdet_stem_conv_pool_fwd(const void* x, const void* w_packed, const float* bias, void* y, int n, int h, int w,
                             int cout, int k, int conv_pad_mode, int pool_pad_mode, int dtype, sqdet_stream_t stream);
/* The same ending with the NEXT layer's squeeze1x1 (fire2/squeeze1x1 of SqueezeDet: 64 -> 16 couts, ReLU,
 * nets/squeezeDet.py:46 via :95-97): pool1's tensor is never written, only the squeeze tensor sq_out [n, Hp, Wp, next_s]
 * (120 MB -> 30 MB at batch 32).  float16, k = 3, cout = 64, even w; w_next_s_packed from sqdet_conv_pack_weights(1, cout,
 * next_s).  Same values as the separate launches (the pooled pixels are rounded to float16 before the squeeze, the
 * squeeze accumulates its two K-chunks in ascending order). */
int sqdet_stem_conv_pool_squeeze_supported(int h, int w, int cout, int k, int conv_pad_mode, int pool_pad_mode, int next_s,
                                           int dtype, int n);
int sqdet_stem_conv_pool_squeeze_fwd(const void* x, const void* w_packed, const float* bias, const void* w_next_s_packed,
                                     const float* b_next_s, void* sq_out, int n, int h, int w, int cout, int k,
                                     int conv_pad_mode, int pool_pad_mode, int next_s, int dtype, sqdet_stream_t stream);

/* ------------------------------------------------------------------ fire --
 * Replaces SqueezeDet._fire_layer (nets/squeezeDet.py:81-106):
 *   sq = relu(conv1x1(x)); y = concat(relu(conv1x1(sq)), relu(conv3x3(sq))).
 * w_* are packed kernels; sq_scratch: [n,h,w,s1x1] scratch in dtype storage.
 * Every sqdet_fire_*_fwd call below refuses a NULL operand (scratches included) and non-positive n / h / w / channel counts
 * with SQDET_EINVAL before anything is launched, as sqdet_conv2d_nhwc_fwd does; nothing is written then. */
int sqdet_fire_fwd(const void* x, const void* w_s, const float* b_s, const void* w_e1, const float* b_e1,
                   const void* w_e3, const float* b_e3, void* sq_scratch, void* y,
                   int n, int h, int w, int cin, int s1x1, int e1x1, int e3x3, int dtype, sqdet_stream_t stream);
/* sqdet_fire_fwd that ALSO leaves the module's squeeze tensor relu(conv1x1(x)) in sq_out [n,h,w,s1x1] (training: the
 * module's backward reads it); the fused kernels write it from their squeeze epilogue -- still one launch. */
int sqdet_fire_fwd_keep(const void* x, const void* w_s, const float* b_s, const void* w_e1, const float* b_e1,
                        const void* w_e3, const float* b_e3, void* sq_out, void* y, int n, int h, int w,
                        int cin, int s1x1, int e1x1, int e3x3, int dtype, sqdet_stream_t stream);

/* Fire module followed by max_pool 3x3 / stride 2 / SAME (fire3 -> pool3, fire5 -> pool5: nets/squeezeDet.py:49-57)
 * in one launch where the streaming kernel covers the shape: the pool is taken in registers and only the pooled
 * tensor y [n, ceil(h/2), ceil(w/2), e1x1+e3x3] is written.  fire_scratch [n,h,w,e1x1+e3x3] and sq_scratch (as in
 * sqdet_fire_fwd) are only used by the unfused fallback.  Results are bitwise those of fire -> pool. */
int sqdet_fire_maxpool_fwd(const void* x, const void* w_s, const float* b_s, const void* w_e1, const float* b_e1,
                           const void* w_e3, const float* b_e3, void* sq_scratch, void* fire_scratch, void* y,
                           int n, int h, int w, int cin, int s1x1, int e1x1, int e3x3, int dtype, sqdet_stream_t stream);

/* The expand half of a fire module from its squeeze tensor sq_in [n,h,w,s1x1] (produced by a chain launch, below):
 *   y = concat(relu(conv1x1(sq_in, W_e1) + b_e1), relu(conv3x3(sq_in, W_e3) + b_e3))     (nets/squeezeDet.py:92-106),
 * pool != 0: followed by max_pool 3x3 / stride 2 / SAME (fire3 -> pool3, fire5 -> pool5: nets/squeezeDet.py:49-57) taken
 * in registers -- y is then the pooled tensor [n, ceil(h/2), ceil(w/2), e1x1+e3x3] (float16 shapes of the streaming
 * kernel only).  w_e1 / w_e3: packed by sqdet_conv_pack_weights.  Bitwise sqdet_fire_fwd / sqdet_fire_maxpool_fwd.
 * Deep squeezes (SqueezeDet+: 192 / 384 channels, nets/squeezeDetPlus.py:46-73), pool == 0: ONE launch of the 3x3 tile kernel that
 * also runs the expand1x1 on the staged squeeze tile where sqdet_fire_expand_pair_supported says 1 (float16, e1x1 == e3x3 a multiple
 * of 64 >= 128, the halo tile resident in LDS); two conv launches otherwise.  Bitwise the two convs either way. */
int sqdet_fire_expand_pair_supported(int n, int h, int w, int s1x1, int e1x1, int e3x3, int dtype);
int sqdet_fire_expand_fwd(const void* sq_in, const void* w_e1, const float* b_e1, const void* w_e3, const float* b_e3,
                          void* y, int n, int h, int w, int s1x1, int e1x1, int e3x3, int pool, int dtype,
                          sqdet_stream_t stream);

/* A whole fire module from its input x [n,h,w,cin] whose concat tensor is replaced by the NEXT module's squeeze tensor
 * sq_out [n,h,w,next_s1x1] = relu(conv1x1(fire(x), W_next_s) + b_next_s)  (fire2 -> fire3's squeeze, fire4 -> fire5's squeeze:
 * nets/squeezeDet.py:46-53, 81-106): the streaming kernel keeps the module's rounded float16 results in an LDS tile and
 * runs the next squeeze on it.  All kernels packed by sqdet_conv_pack_weights.  Bitwise sqdet_fire_fwd followed by the
 * squeeze conv.  sqdet_fire_squeeze_next_supported: 1 when the shape is covered (float16, SqueezeDet's two pairs). */
int sqdet_fire_squeeze_next_supported(int cin, int s1x1, int e1x1, int e3x3, int next_s1x1, int dtype);
int sqdet_fire_squeeze_next_fwd(const void* x, const void* w_s, const float* b_s, const void* w_e1, const float* b_e1,
                                const void* w_e3, const float* b_e3, const void* w_next_s, const float* b_next_s, void* sq_out,
                                int n, int h, int w, int cin, int s1x1, int e1x1, int e3x3, int next_s1x1, int dtype,
                                sqdet_stream_t stream);

/* The expand half of a module from its squeeze tensor (+ max_pool 3x3/s2/SAME when pool != 0) whose output is the NEXT
 * module's squeeze tensor sq_out [n, h', w', next_s1x1] (h', w' = pooled dims when pool): fire3+pool3 -> fire4's squeeze,
 * fire4 -> fire5's, fire5+pool5 -> fire6's (nets/squeezeDet.py:49-58).  Bitwise sqdet_fire_expand_fwd + the squeeze conv. */
int sqdet_fire_expand_squeeze_next_supported(int s1x1, int e1x1, int e3x3, int next_s1x1, int pool, int dtype);
int sqdet_fire_expand_squeeze_next_fwd(const void* sq_in, const void* w_e1, const float* b_e1, const void* w_e3, const float* b_e3,
                                       const void* w_next_s, const float* b_next_s, void* sq_out, int n, int h, int w, int s1x1,
                                       int e1x1, int e3x3, int next_s1x1, int pool, int dtype, sqdet_stream_t stream);

/* Fire-module CHAIN (float16): the expand half of one fire module and the squeeze of the NEXT module in one launch.
 * Replaces, for consecutive fire modules on one feature map (fire6 .. fire11, nets/squeezeDet.py:58-69), the pair
 *   e = concat(relu(conv1x1(sq_in, W_e1) + b_e1), relu(conv3x3(sq_in, W_e3) + b_e3))      (nets/squeezeDet.py:92-106)
 *   sq_out = relu(conv1x1(e, W_next_s) + b_next_s)                                          (the next module's :86-90)
 * sq_in: [n,h,w,s1x1] = the module's own squeeze tensor; the concat tensor e [n,h,w,e1x1+e3x3] is written only when
 * y != NULL; sq_out [n,h,w,next_s1x1] only when next_s1x1 > 0 (at least one of the two).  The three kernels travel as
 * ONE packed weight stream (sqdet_fire_chain_pack: float32 HWIO in, any of the three may be NULL = that part of the
 * stream is left as it is); sqdet_fire_chain_stream_bytes returns 0 for shapes the kernel does not cover
 * (float16 only; s1x1 in 8..96 step 8, e1x1 / e3x3 multiples of 64, next_s1x1 in {0,16,32,48} behind a squeeze of up to
 * 32 channels, {0,48,64,96} behind a wider one -- sqdet_fire_chain_fwd returns SQDET_EUNSUPPORTED exactly where the byte count
 * is 0).  Results are bitwise
 * those of sqdet_fire_fwd followed by the next module's squeeze conv. */
size_t sqdet_fire_chain_stream_bytes(int s1x1, int e1x1, int e3x3, int next_s1x1, int dtype);
int sqdet_fire_chain_pack(const float* w_e1_hwio, const float* w_e3_hwio, const float* w_next_s_hwio, void* stream_buf,
                          int s1x1, int e1x1, int e3x3, int next_s1x1, int dtype, sqdet_stream_t stream);
int sqdet_fire_chain_fwd(const void* sq_in, const void* stream_buf, const float* b_e1, const float* b_e3,
                         const float* b_next_s, void* y, void* sq_out, int n, int h, int w, int s1x1, int e1x1,
                         int e3x3, int next_s1x1, int dtype, sqdet_stream_t stream);

/* ---------------------------------------------------- interpret_output --
 * Replaces ModelSkeleton._add_interpretation_graph (nn_skeleton.py:142-283) +
 * util.safe_exp / bbox_transform / bbox_transform_inv (utils/util.py:167-231).
 * preds: [n,gh,gw,apg*(classes+1+4)] (dtype storage); anchors: float32
 * [gh*gw*apg,4] = float32(mc.ANCHOR_BOX).  Outputs (all [n,A,...], A=gh*gw*apg):
 * det_boxes float32 [n,A,4] (cx,cy,w,h), det_probs float32 [n,A], det_class
 * int64 [n,A]; optional (may be NULL) pred_class_probs float32 [n,A,classes],
 * pred_conf float32 [n,A].  Separate mul/add float32 ops (no FMA contraction). */
int sqdet_interpret_output(const void* preds, const float* anchors, float* det_boxes, float* det_probs,
                           int64_t* det_class, float* pred_class_probs, float* pred_conf,
                           int n, int gh, int gw, int apg, int classes, float img_w, float img_h, float exp_thresh,
                           int dtype, sqdet_stream_t stream);

/* --------------------------------------------------- filter_prediction --
 * Replaces ModelSkeleton.filter_prediction (nn_skeleton.py:696-734) +
 * util.nms / util.batch_iou (utils/util.py:32-76), batched over n images.
 * Inputs: boxes float32 [n,A,4] (cx,cy,w,h), probs float32 [n,A], cls int64 [n,A].
 * top_n > 0 and < A: the top_n highest probs (ties: higher anchor index first)
 *   enter NMS, prob_thresh is ignored (nn_skeleton.py:711-715);
 * otherwise: entries with prob > prob_thresh enter NMS (nn_skeleton.py:716-720).
 * NMS is the reference's NON-greedy rule: j is dropped iff some same-class i
 * with higher prob has (double)IoU(i,j) > nms_thresh.
 * Outputs, capacity max_out per image (>= top_n in the top-N branch), ordered
 * by class then descending prob: out_boxes float32 [n,max_out,4], out_probs
 * float32 [n,max_out], out_cls int32 [n,max_out], out_index int32 [n,max_out]
 * (anchor index), out_count int32 [n] (number of valid rows; if the threshold
 * branch yields more than max_out candidates the call reports it through
 * out_count[i] = -(number of candidates)). */
int sqdet_filter_prediction(const float* boxes, const float* probs, const int64_t* cls,
                            float* out_boxes, float* out_probs, int32_t* out_cls, int32_t* out_index,
                            int32_t* out_count, int n, int num_anchors, int classes, int top_n, int max_out,
                            double nms_thresh, float prob_thresh, sqdet_stream_t stream);

/* interpret_output + filter_prediction in ONE call (two launches: scores chip-wide, then one workgroup per image) for the top-N branch (0 < top_n <= 64 < A <= 20480: every reference
 * config): the scores of all anchors are computed on the fly, boxes and classes are decoded for the <= top_n selected
 * anchors only -- det_boxes / det_class (0.47 MB per image in the reference's sess.run) never exist.  Same float
 * expressions as sqdet_interpret_output, same selection / NMS as sqdet_filter_prediction: identical outputs.
 * scratch_probs: float32 [n, A] device scratch (det_probs; read back only when more than 2048 anchors tie at the top-N
 * boundary).  Outputs as sqdet_filter_prediction. */
int sqdet_detect_filter(const void* preds, const float* anchors, float* scratch_probs, float* out_boxes, float* out_probs,
                        int32_t* out_cls, int32_t* out_index, int32_t* out_count, int n, int gh, int gw, int apg, int classes,
                        float img_w, float img_h, float exp_thresh, int top_n, int max_out, double nms_thresh, int dtype,
                        sqdet_stream_t stream);

/* sqdet_detect_filter with the scores already computed (sqdet_convdet_fwd / sqdet_net_set_scores: det_probs float32 [n, A]):
 * the filter launch only.  Identical outputs.  max_workgroups > 0: the n images are walked by at most that many workgroups
 * (<= 0: one per image) -- a serving loop that overlaps this launch with the next batch's forward sizes it to the CUs that
 * forward leaves idle (16 during SqueezeDet's fire6..fire11 launches at batch 32). */
int sqdet_detect_filter_scored(const void* preds, const float* anchors, const float* scores, float* out_boxes, float* out_probs,
                               int32_t* out_cls, int32_t* out_index, int32_t* out_count, int n, int gh, int gw, int apg,
                               int classes, float img_w, float img_h, float exp_thresh, int top_n, int max_out,
                               double nms_thresh, int dtype, int max_workgroups, sqdet_stream_t stream);

/* A second suppression stage over the rows a filter call above emitted (OURS): greedy NMS, Soft-NMS (linear /
 * Gaussian), DIoU-NMS and class-agnostic suppression.  The filter is called with nms_thresh = +inf (it then only selects and
 * orders the top-N rows); this call applies the rule IN PLACE on its five outputs: boxes float32 [n,rows,4] (cx,cy,w,h), probs
 * float32 [n,rows], cls int32 [n,rows], index int32 [n,rows], count int32 [n]; 1 <= rows <= 64.  One launch, one workgroup per
 * image.  Rows are ranked by (prob, anchor index) descending -- the filter's own total order.
 *   method   NONGREEDY: r is dropped iff some higher-ranked i has (double)ov(i,r) > nms_thresh (sqdet_filter_prediction's rule);
 *            GREEDY: the same, but only a kept i suppresses; SOFT_LINEAR / SOFT_GAUSSIAN (Bodla et al. 2017), float64 scores
 *            starting at prob: pick the remaining row of the largest score (ties: higher rank), stop when it is < score_floor,
 *            keep it, then decay every remaining row j under the class test: linear s_j *= 1 - iou where (double)iou >
 *            nms_thresh; Gaussian s_j *= exp(-(iou*iou) / sigma) for every j.  The output prob is (float)s.
 *   overlap  IOU: the filter's float32 IoU; DIOU (Zheng et al. 2020; hard methods only), in float64: iou - d^2 / c^2 with d the
 *            centre distance and c the diagonal of the enclosing box.  A NaN overlap never suppresses.
 *   class_agnostic  != 0: rows of different classes suppress / decay each other too.
 * Output as the filter's: kept rows ordered by class, then pick order; rows [kept, rows) zeroed (boxes 0, prob 0, cls -1,
 * index -1); count = kept.  An image whose count is outside [0, rows] (the filter's overflow report) is left untouched.
 * NULL pointers, rows outside 1..64, an unknown method / overlap, DIOU with a soft method, sigma <= 0 or a non-finite
 * score_floor: SQDET_EINVAL, nothing launched. */
enum { SQDET_NMS_NONGREEDY = 0, SQDET_NMS_GREEDY = 1, SQDET_NMS_SOFT_LINEAR = 2, SQDET_NMS_SOFT_GAUSSIAN = 3 };
enum { SQDET_NMS_OVERLAP_IOU = 0, SQDET_NMS_OVERLAP_DIOU = 1 };
typedef struct { int method; int overlap; int class_agnostic; double nms_thresh; double sigma; double score_floor; } sqdet_nms_options_t;
int sqdet_suppress_rows(float* boxes, float* probs, int32_t* cls, int32_t* index, int32_t* count, int n, int rows, int classes,
                        const sqdet_nms_options_t* opt, sqdet_stream_t stream);

/* ------------------------------------------------------------ training --
 * Replaces the gradient half of the reference's TF graph for the trainable convs (stride 1,
 * SAME: every conv but the frozen conv1, nets/squeezeDet.py:40-42), the loss graph
 * (ModelSkeleton._add_loss_graph, nn_skeleton.py:285-327, on top of _add_interpretation_graph
 * :142-283) and the train graph (ModelSkeleton._add_train_graph, nn_skeleton.py:329-361).
 * float32 storage (SQDET_F32) is the reference's training dtype; the activation-side kernels also take
 * SQDET_F16 (mixed precision: float16 activations / activation gradients with loss scaling, float32
 * master weights, weight gradients and optimizer -- BASELINE.json configs[4] "fp16 training").
 */

/* MANY kernels packed in ONE launch (a training step re-packs every trainable conv kernel twice after the optimizer step:
 * forward fragment order = sqdet_conv_pack_weights, backward-data order = sqdet_conv_pack_weights_bwd_data; 62 launches in
 * SqueezeDet's step).  sqdet_conv_pack_many_prepare fills a HOST table of sqdet_conv_pack_many_table_bytes(n) bytes from
 * per-item arrays (device pointers of the float32 HWIO kernels and of the packed outputs, k / cin / cout, bwd_data flags)
 * and reports the grid; the caller copies the table to the device once; sqdet_conv_pack_many runs it (same bytes as the
 * per-kernel entry points produce: one index decomposition and one element fetch per order under all three kernels). */
size_t sqdet_conv_pack_many_table_bytes(int nitems);
int sqdet_conv_pack_many_prepare(const float* const* w_hwio_f32, void* const* packed, const int* k, const int* cin, const int* cout,
                                 const int* bwd_data, int nitems, int dtype, void* table_host, int* total_blocks);
/* With the batch norm of _conv_bn_layer convs folded on the way (items whose gamma[i] != NULL): what is packed is
 * W[..., c] * gamma[c] / sqrt(var[c] + eps) -- sqdet_fold_batchnorm (its scale and bias expressions themselves) followed by
 * the packer, bit for bit, without the folded float32 kernel ever being written -- and b_folded[i] (when not NULL) receives the folded bias.  The pointer arrays may be
 * NULL altogether (= sqdet_conv_pack_many_prepare). */
int sqdet_conv_pack_many_prepare_bn(const float* const* w_hwio_f32, void* const* packed, const int* k, const int* cin,
                                    const int* cout, const int* bwd_data, const float* const* gamma, const float* const* beta,
                                    const float* const* mean, const float* const* var, const float* const* conv_bias,
                                    float* const* b_folded, float eps, int nitems, int dtype, void* table_host, int* total_blocks);
int sqdet_conv_pack_many(const void* table_dev, int nitems, int total_blocks, int dtype, sqdet_stream_t stream);

/* Backward-data: dx = conv(dy, rot180(W)^T).  pack: float32 HWIO [k,k,cin,cout] -> fragment order
 * of the [k,k,cout,cin] kernel (same size as sqdet_conv_packed_bytes(k, cout, cin, dtype)).
 * dy is channels [dy_coffset, +cout) of rows dy_cstride wide (a fire module's concat gradient);
 * accumulate != 0: dx += result (the squeeze tensor receives expand1x1's and expand3x3's dgrad). */
int sqdet_conv_pack_weights_bwd_data(const float* w_hwio_f32, void* packed, int k, int cin, int cout, int dtype,
                                     sqdet_stream_t stream);
int sqdet_conv2d_nhwc_bwd_data(const void* dy, const void* w_packed_bwd, void* dx, int n, int h, int w, int cin,
                               int cout, int k, int dtype, int dy_cstride, int dy_coffset, int accumulate,
                               sqdet_stream_t stream);
/* The same with the ReLU backward of the layer below in the epilogue: dx is the gradient w.r.t. the ReLU output
 * relu_of [n,h,w,cin] (the conv's input in the forward pass) and is zeroed where relu_of <= 0 -- after the
 * accumulation when accumulate != 0 (tf.nn.relu's gradient, nn_skeleton.py:547 through tf.gradients) -- instead of a
 * separate sqdet_relu_bwd pass over the tensor. */
int sqdet_conv2d_nhwc_bwd_data_relu(const void* dy, const void* w_packed_bwd, void* dx, const void* relu_of, int n, int h,
                                    int w, int cin, int cout, int k, int dtype, int dy_cstride, int dy_coffset,
                                    int accumulate, sqdet_stream_t stream);

/* Backward-filter (+ bias): dW[kh,kw,ci,co] = grad_scale * sum_pixels x@tap[ci]*dy[co] (+ weight_decay*W
 * when w_hwio_for_decay != NULL: the gradient of wd*l2_loss(W), nn_skeleton.py:66-69), dbias[co] =
 * grad_scale * sum dy (dbias may be NULL).  x / dy (dtype SQDET_F32 or SQDET_F16) may be channel slices;
 * dW / dbias are float32 either way; grad_scale = 1, or 1/loss_scale in mixed-precision training.
 * workspace: device scratch of sqdet_conv2d_bwd_filter_workspace_bytes(...).  Deterministic (two-pass
 * slab reduction, no atomics). */
size_t sqdet_conv2d_bwd_filter_workspace_bytes(int n, int h, int w, int cin, int cout, int k);
int sqdet_conv2d_nhwc_bwd_filter(const void* x, const void* dy, float* dw_hwio, float* dbias,
                                 const float* w_hwio_for_decay, float weight_decay, float grad_scale, float* workspace,
                                 int n, int h, int w, int cin, int cout, int k, int x_cstride, int x_coffset,
                                 int dy_cstride, int dy_coffset, int dtype, sqdet_stream_t stream);
/* The two halves apart, for a step that takes MANY weight gradients: sqdet_conv2d_nhwc_bwd_filter_partial writes only the
 * partial slabs of one conv into its own workspace (same size query), and ONE sqdet_slab_reduce_many launch at the end of
 * the backward pass sums the slabs of all of them (a SqueezeDet step: 31 reductions, each a 10 us launch behind its
 * gradient kernel).  prepare() fills a host table (sqdet_slab_reduce_many_table_bytes(n_items) bytes; the caller copies it
 * to the device once) from the per-item workspace / dW / dbias (NULL: none) / decay-weight (NULL: none) pointers and the
 * conv shapes the partial launches used; per item the reduction is sqdet_conv2d_nhwc_bwd_filter's own device code on that
 * item's block count, so its bits. */
int sqdet_conv2d_nhwc_bwd_filter_partial(const void* x, const void* dy, float* workspace, int want_bias, int n, int h, int w,
                                         int cin, int cout, int k, int x_cstride, int x_coffset, int dy_cstride,
                                         int dy_coffset, int dtype, sqdet_stream_t stream);
size_t sqdet_slab_reduce_many_table_bytes(int n_items);
int sqdet_slab_reduce_many_prepare(const float* const* workspaces, float* const* dws, float* const* dbiases,
                                   const float* const* w_for_decay, const float* decays, const int* n, const int* h,
                                   const int* w, const int* cin, const int* cout, const int* k, int n_items,
                                   void* table_host, int* total_blocks);
int sqdet_slab_reduce_many(const void* table_dev, int n_items, int total_blocks, float grad_scale, sqdet_stream_t stream);

/* dy *= (y > 0)  (tf.nn.relu gradient; count elements, a multiple of 16 bytes). */
int sqdet_relu_bwd(const void* y, void* dy_inout, size_t count, int dtype, sqdet_stream_t stream);
/* y = x * mask * scale: tf.nn.dropout forward (mask = floor(keep_prob + U) in {0,1}, scale =
 * 1/keep_prob; nets/squeezeDet.py:74) and its backward.  x, mask, y share dtype. */
int sqdet_scale_mask(const void* x, const void* mask, void* y, float scale, size_t count, int dtype,
                     sqdet_stream_t stream);
/* The same with the ReLU backward of the layer below in the same pass: y = relu_of > 0 ? x * mask * scale : 0 (relu_of: the
 * ReLU output x is the gradient of -- fire11's output under the dropout in front of conv12). */
int sqdet_scale_mask_relu(const void* x, const void* mask, const void* relu_of, void* y, float scale, size_t count, int dtype,
                          sqdet_stream_t stream);
/* dst[i] = (dst_dtype)(src[i] * scale): the float16 <-> float32 hand-offs of mixed-precision training (float16
 * preds -> the float32 loss kernel; its float32 dpreds * loss_scale -> float16).  count a multiple of 4. */
int sqdet_convert_scale(const void* src, int src_dtype, void* dst, int dst_dtype, float scale, size_t count,
                        sqdet_stream_t stream);
/* tf.nn.max_pool gradient: dx[cell] = sum of dy over the windows whose first maximum the cell is. */
int sqdet_maxpool_nhwc_bwd(const void* x, const void* dy, void* dx, int n, int h, int w, int c, int k, int stride,
                           int pad_mode, int dtype, sqdet_stream_t stream);
/* The same for a pool whose input x is a ReLU output (every pool of the reference's trained nets): dx is also zeroed where
 * x <= 0, i.e. the ReLU backward of the layer below is taken here instead of in a pass of its own. */
int sqdet_maxpool_nhwc_bwd_relu(const void* x, const void* dy, void* dx, int n, int h, int w, int c, int k, int stride,
                                int pad_mode, int dtype, sqdet_stream_t stream);
/* Both from the window index of sqdet_maxpool_nhwc_fwd_idx (k = 3 or 2, stride 2) instead of x: reads three quarter-size
 * maps (index, dy and -- relu != 0 -- the pooled y, whose sign is the sign of x at every cell that receives anything)
 * and writes every cell of dx [n,h,w,c] (cells no window covers: zero); bitwise the results of the two functions above. */
int sqdet_maxpool_nhwc_bwd_idx(const unsigned char* window_index, const void* y, const void* dy, void* dx, int n, int h,
                               int w, int c, int k, int stride, int pad_mode, int dtype, int relu, sqdet_stream_t stream);

/* Loss forward + backward.  Inputs as the reference's placeholders (nn_skeleton.py:86-97):
 * input_mask [B,A], box_delta_input [B,A,4], box_input [B,A,4] (cx,cy,w,h), labels [B,A,C];
 * num_objects = sum(input_mask) over the batch.  Outputs: dpreds = d(class+conf+bbox loss)/dpreds
 * [B,gh,gw,K*(C+5)], ious [B,A] (the assign'ed IoU target, no gradient), losses3 = {class_loss,
 * conf_loss, bbox_loss}.  workspace: sqdet_loss_workspace_bytes() of device scratch.
 * global_batch: the divisor of the confidence term's reduce_mean over the batch (nn_skeleton.py:304-312); <= 0 = `batch`.
 * Data-parallel replicas that reproduce ONE graph of batch world*B (num_objects all-reduced, gradients SUMMED) pass
 * world*B here: the class / bbox terms divide by num_objects only, the confidence term also by the batch. */
size_t sqdet_loss_workspace_bytes(void);
int sqdet_loss_fwd_bwd(const float* preds, const float* anchors, const float* input_mask, const float* box_delta_input,
                       const float* box_input, const float* labels, float* dpreds, float* ious, float* losses3,
                       float* workspace, int batch, int gh, int gw, int apg, int classes, float img_w, float img_h,
                       float exp_thresh, float epsilon, float coef_class, float coef_conf_pos, float coef_conf_neg,
                       float coef_bbox, float num_objects, int global_batch, sqdet_stream_t stream);

/* Same, with num_objects read from the DEVICE (float32 scalar, e.g. sqdet_sum_f32 of input_mask -- nn_skeleton.py:180 --
 * optionally SUM-all-reduced over the replicas first: the exact global-batch normalisation of SURVEY.md 8e option b):
 * no device -> host round trip, so the whole step can be captured in a hipGraph. */
int sqdet_loss_fwd_bwd_dev(const float* preds, const float* anchors, const float* input_mask, const float* box_delta_input,
                           const float* box_input, const float* labels, float* dpreds, float* ious, float* losses3,
                           float* workspace, int batch, int gh, int gw, int apg, int classes, float img_w, float img_h,
                           float exp_thresh, float epsilon, float coef_class, float coef_conf_pos, float coef_conf_neg,
                           float coef_bbox, const float* num_objects_dev, int global_batch, sqdet_stream_t stream);

/* Mixed-precision form: preds are FLOAT16 (read as their float32 values) and, beside the float32 dpreds, the loss-scaled
 * float16 gradient the float16 backward starts from is written in the same pass -- (float16)(dpreds * loss_scale), the
 * expression of sqdet_convert_scale -- instead of a conversion launch either side of the loss.  num_objects_dev != NULL:
 * the count is read from the device (num_objects ignored). */
int sqdet_loss_fwd_bwd_mixed(const void* preds_f16, const float* anchors, const float* input_mask, const float* box_delta_input,
                             const float* box_input, const float* labels, float* dpreds, void* dpreds_scaled_f16,
                             float loss_scale, float* ious, float* losses3, float* workspace, int batch, int gh, int gw, int apg,
                             int classes, float img_w, float img_h, float exp_thresh, float epsilon, float coef_class,
                             float coef_conf_pos, float coef_conf_neg, float coef_bbox, float num_objects,
                             const float* num_objects_dev, int global_batch, sqdet_stream_t stream);

/* The loss with options (OURS): one function for float32 preds (preds_dtype SQDET_F32; dpreds_scaled_f16 and
 * loss_scale ignored) and float16 preds (SQDET_F16: the mixed form above, both gradients written in one pass), for the host
 * num_objects and -- num_objects_dev != NULL -- the device one, and for global_batch.
 *   box_loss     what replaces the squared error on the four deltas: coef_bbox * sum_a m * (1 - X) / num_objects with X the
 *                IoU / GIoU / DIoU / CIoU of the decoded, clipped box (the corners `ious` is formed on) and the ground truth.
 *   focal_gamma  g > 0: the class term lab * (1-pc)^g * (-log(pc+eps)) + (1-lab) * pc^g * (-log(1-pc+eps)).
 * Gradients are the exact chain rule through the corner form, the clip to the image, safe_exp's two branches and the
 * softmax; CIoU's alpha is a constant in the backward pass.  Tie rule: a coordinate of the prediction receives gradient
 * through a min / max / clip only where it is strictly the selected argument -- at equality the ground truth's coordinate,
 * the 0 of the intersection's max(0, .) or the image border takes it; an edge exactly on the border counts as clipped.
 * `ious` stays the plain IoU, losses3 keeps its three slots, the reductions their fixed order.
 * {SQDET_BOX_LOSS_DELTA_L2, 0} returns the bits of the three functions above (it calls them).  A box_loss outside 0..4 or a
 * negative / non-finite focal_gamma: SQDET_EINVAL, nothing launched. */
enum { SQDET_BOX_LOSS_DELTA_L2 = 0, SQDET_BOX_LOSS_IOU = 1, SQDET_BOX_LOSS_GIOU = 2, SQDET_BOX_LOSS_DIOU = 3, SQDET_BOX_LOSS_CIOU = 4 };
typedef struct { int box_loss; float focal_gamma; } sqdet_loss_options_t;
int sqdet_loss_fwd_bwd_opt(const void* preds, int preds_dtype, const float* anchors, const float* input_mask,
                           const float* box_delta_input, const float* box_input, const float* labels, float* dpreds,
                           void* dpreds_scaled_f16, float loss_scale, float* ious, float* losses3, float* workspace, int batch,
                           int gh, int gw, int apg, int classes, float img_w, float img_h, float exp_thresh, float epsilon,
                           float coef_class, float coef_conf_pos, float coef_conf_neg, float coef_bbox, float num_objects,
                           const float* num_objects_dev, int global_batch, const sqdet_loss_options_t* opt,
                           sqdet_stream_t stream);
/* ---- distillation (OURS): a teacher net's ConvDet output as a second target of the loss.
 * preds (the student's) and teacher_preds are [B,gh,gw,K*(C+5)] with loss_kernel's channels: class logits at k*C + c, the
 * confidence logit at K*C + k, the four deltas at K*(C+1) + 4k + d.  Per anchor a of image b, with the student's values zs, us, ds
 * and the teacher's zt, ut, dt, A = gh*gw*K anchors per image and Bg = global_batch (<= 0: batch; as in sqdet_loss_fwd_bwd):
 *   ct = sigmoid(ut), cs = sigmoid(us);  w = ct if ct >= conf_floor (inclusive), else 0 -- a constant of the backward pass.
 *   class  q = softmax(zt/T), p = softmax(zs/T), through the max-subtracted log-softmax lq, lp:
 *          L_cls  = class_coef * T^2 / Bg * sum_{b,a} w * sum_j q_j (lq_j - lp_j);    dL/dzs_j = class_coef * T * w * (p_j - q_j) / Bg
 *   conf   the Bernoulli KL in logit form, softplus(z) = max(z,0) + log1p(exp(-|z|)):
 *          L_conf = conf_coef / (Bg*A) * sum_{b,a} [ ct (ut - us) + softplus(us) - softplus(ut) ];   dL/dus = conf_coef * (cs - ct) / (Bg*A)
 *   box    L_box  = bbox_coef / Bg * sum_{b,a} w * sum_d (ds_d - dt_d)^2;             dL/dds_d = 2 bbox_coef w (ds_d - dt_d) / Bg
 * No normaliser depends on the data: a data-parallel replica's share needs no all-reduce of its own.  The teacher gets no
 * gradient; non-finite teacher values are UNDEFINED behaviour of the arithmetic (the caller's problem).
 * The call runs AFTER the loss launch that wrote dpreds_inout: every channel's gradient g is computed completely, then
 * dpreds = dpreds + g (one float32 add) and -- float16 student -- dpreds_scaled_f16 = (float16)(dpreds * loss_scale) on that sum,
 * sqdet_convert_scale's expression, in the same pass.  distill3 = {class, conf, box} term; workspace:
 * sqdet_distill_workspace_bytes() of device scratch.  preds_dtype / teacher_dtype: SQDET_F32 or SQDET_F16, any pair; the
 * arithmetic is float32 on the stored values.  Deterministic (fixed-order sums, no atomics), capturable in a hipGraph.
 * SQDET_EINVAL, nothing launched: temperature <= 0 or non-finite, a negative or non-finite coefficient, all three coefficients
 * zero, conf_floor outside [0, 1], an unknown dtype, float16 preds without dpreds_scaled_f16 / a loss scale > 0. */
typedef struct { float temperature, class_coef, conf_coef, bbox_coef, conf_floor; } sqdet_distill_options_t;
size_t sqdet_distill_workspace_bytes(void);
int sqdet_distill_fwd_bwd(const void* preds, int preds_dtype, const void* teacher_preds, int teacher_dtype, float* dpreds_inout,
                          void* dpreds_scaled_f16, float loss_scale, float* distill3, float* workspace, int batch, int gh, int gw,
                          int apg, int classes, int global_batch, const sqdet_distill_options_t* opt, sqdet_stream_t stream);
/* out[0] = sum(x[0..count)) in a fixed order (deterministic): tf.reduce_sum(self.input_mask), nn_skeleton.py:180. */
int sqdet_sum_f32(const float* x, size_t count, float* out, sqdet_stream_t stream);
/* y = max(a + b, 0): tf.nn.relu(shortcut + branch) (nets/resnet50_convDet.py:55) where the producing conv could not take
 * the add in its epilogue.  count elements, a multiple of 16 bytes; y may alias a or b. */
int sqdet_add_relu(const void* a, const void* b, void* y, size_t count, int dtype, sqdet_stream_t stream);
/* y[p, y_coffset .. +c) = x[p, 0 .. c) for `pixels` rows: one input of tf.concat(values, 3) (nets/squeezeDet.py:106) whose
 * producer could not write its channel range directly.  c, y_cstride, y_coffset multiples of 16 bytes. */
int sqdet_copy_channels(const void* x, void* y, size_t pixels, int c, int y_cstride, int y_coffset, int dtype,
                        sqdet_stream_t stream);
/* mask[i] = min(floor(keep_prob + u_i), 1), u_i ~ U[0,1) in 24 bits from a counter-based generator of (seed, i): the keep
 * mask of tf.nn.dropout (nets/squeezeDet.py:74), every element 0 or 1 (the min only acts at keep_prob = 1, where the float32
 * sum 1 + (1 - 2^-24) rounds to 2), to be applied with sqdet_scale_mask(x, mask, 1/keep_prob). */
int sqdet_dropout_mask(void* mask, size_t count, float keep_prob, uint64_t seed, int dtype, sqdet_stream_t stream);

/* Momentum + per-variable clip_by_norm over flat parameter / gradient / momentum buffers.
 * Variable v = elements [offsets[v], +counts[v]); decays[v] = weight decay added to its gradient
 * BEFORE clipping (0 for biases).  step: g = g*grad_scale (1/world_size after a SUM all-reduce) + decay*w; g *= max_norm/max(||g||,max_norm);
 * accum = momentum*accum + g; w -= lr*accum.  Deterministic (fixed-order norm reduction), so
 * data-parallel replicas stay bit-identical.  found_inf (device int32, may be NULL): set to 1 when any
 * variable's gradient norm is inf / NaN -- the step is then skipped entirely (params and accum untouched;
 * the overflow case of loss-scaled float16 training) -- else 0. */
typedef struct sqdet_optimizer sqdet_optimizer_t;
int sqdet_optimizer_create(sqdet_optimizer_t** out, const long* offsets, const long* counts, const float* decays,
                           int nvars);
void sqdet_optimizer_destroy(sqdet_optimizer_t* opt);
size_t sqdet_optimizer_workspace_bytes(const sqdet_optimizer_t* opt);
int sqdet_optimizer_step(sqdet_optimizer_t* opt, float* params, float* grads, float* accum, void* workspace, float lr,
                         float momentum, float max_grad_norm, float grad_scale, int32_t* found_inf,
                         sqdet_stream_t stream);

/* The update step with options (OURS): the same three launches over the same segment table and workspace.
 * All element-wise arithmetic is float32, one rounding per operator in the order written; scalars derived per step are formed
 * in float64 and rounded to float32 once.
 *   state   device, 4 doubles: (t, p1, p2, unused) = the number of applied updates, beta1^t and beta2^t as running products
 *           (p1 *= beta1 -- not pow), starting at (0, 1, 1).  A skipped step leaves it untouched.
 *   pass 1  g = g * grad_scale; momentum / nesterov: variables with decay != 0 then get g = g + decay * w (coupled, as above);
 *           adamw: nothing is added.  Per-block float64 partial sums of squares in sqdet_optimizer_step's partition and order.
 *   pass 2  per-variable float64 sums as above; bad = any norm inf / NaN (found_inf, the step is skipped in every buffer).
 *           clip 0: scale[v] = max_norm / fmaxf(n_v, max_norm) (tf.clip_by_norm).  clip 1: the per-variable sums added in
 *           variable-index order, N = (float)sqrt(S), every variable max_norm / fmaxf(N, max_norm) (tf.clip_by_global_norm; a
 *           non-finite N is bad too).  Not bad: t += 1; p1 *= beta1; p2 *= beta2; c1 = (float)(1 / (1 - p1));
 *           c2 = (float)(1 / (1 - p2)); om = (float)(1 - d), d = ema_decay or -- ema_warmup -- min(ema_decay, (1 + t) / (10 + t)).
 *   pass 3  gc = g * scale[v], then
 *           momentum  a = mom*a + gc;  w = w - lr*a                       (the bits of sqdet_optimizer_step)
 *           nesterov  a = mom*a + gc;  w = w - lr*(gc + mom*a)
 *           adamw     m = b1*m + (1-b1)*gc;  v = b2*v + (1-b2)*(gc*gc);  u = (m*c1) / (sqrtf(v*c2) + eps);
 *                     decay != 0: u = u + decay*w;  w = w - lr*u          (m = accum, v = accum2; 1-b1, 1-b2 rounded once)
 *           ema       e = e + om*(w - e), on the value just written.
 * accum2: adamw's second moment, else NULL; ema: NULL without EMA (ema_decay 0).  16-byte vectors where a segment's offset and
 * every base pointer allow it, a scalar path elsewhere -- the same bits; gaps between segments are neither read as data nor
 * written in any buffer.  SQDET_EINVAL, nothing launched: a rule outside 0..2, a clip outside 0..1, accum2 NULL under adamw, ema
 * NULL with ema_decay > 0, momentum / beta1 / beta2 / ema_decay outside [0, 1), eps not finite and positive, a variable's decay
 * negative or non-finite. */
enum { SQDET_OPT_MOMENTUM = 0, SQDET_OPT_NESTEROV = 1, SQDET_OPT_ADAMW = 2 };
enum { SQDET_CLIP_PER_VARIABLE = 0, SQDET_CLIP_GLOBAL = 1 };
typedef struct {
  int rule;            /* SQDET_OPT_* */
  int clip;            /* SQDET_CLIP_* */
  float momentum, beta1, beta2, eps;
  double ema_decay;    /* 0: no EMA */
  int ema_warmup;      /* != 0: d = min(ema_decay, (1 + t) / (10 + t)) */
} sqdet_optimizer_options_t;
int sqdet_optimizer_step_opt(sqdet_optimizer_t* opt, float* params, float* grads, float* accum, float* accum2, float* ema,
                             double* state, void* workspace, float lr, float max_grad_norm, float grad_scale,
                             const sqdet_optimizer_options_t* options, int32_t* found_inf, sqdet_stream_t stream);

/* ------------------------------------------------------------- network --
 * Replaces SqueezeDet.__init__/_add_forward_graph (nets/squeezeDet.py:19-79,
 * nets/squeezeDetPlus.py:19-79) + the sess.run([det_boxes,det_probs,det_class])
 * call shape of demo.py:193-195 / eval.py:75-77.  A net is a host-side plan; its
 * device memory (packed parameters + activation workspace) is caller-owned. */
typedef struct sqdet_net sqdet_net_t;

int sqdet_net_create(sqdet_net_t** out, int arch, int dtype, int batch, int img_h, int img_w, int classes,
                     int anchors_per_grid);
void sqdet_net_destroy(sqdet_net_t* net);

/* Parameters, in graph order, named like the reference's variables
 * ('conv1/kernels', 'fire2/squeeze1x1/biases', ...; nn_skeleton.py:531-536). */
int sqdet_net_num_params(const sqdet_net_t* net);
int sqdet_net_param_info(const sqdet_net_t* net, int index, char* name, size_t name_cap, int shape[4], int* ndim);

size_t sqdet_net_param_bytes(const sqdet_net_t* net);      /* packed kernels + float32 biases */
size_t sqdet_net_workspace_bytes(const sqdet_net_t* net);  /* activation buffers */
int sqdet_net_bind(sqdet_net_t* net, void* param_mem, void* workspace_mem);

/* value: device float32, HWIO for kernels / [cout] for biases.  SQDET_ARCH_RESNET50
 * (nets/resnet50_convDet.py:20-169) also lists '<conv>/gamma', '/beta', '/mean', '/var' for its
 * _conv_bn_layer convs (nn_skeleton.py:427-439); those layers keep the float32 values and fold
 * them into the packed kernel + bias (sqdet_fold_batchnorm) on the next sqdet_net_forward. */
int sqdet_net_set_param(sqdet_net_t* net, const char* name, const float* value_f32, sqdet_stream_t stream);
/* mc.BATCH_NORM_EPSILON (config/config.py:131; default 1e-5). */
int sqdet_net_set_bn_epsilon(sqdet_net_t* net, float eps);

int sqdet_net_output_dims(const sqdet_net_t* net, int* gh, int* gw, int* channels);

/* image_input: [batch,img_h,img_w,3] (dtype storage, BGR mean-subtracted:
 * demo.py:187-190) -> preds [batch,gh,gw,channels] (dtype storage). */
int sqdet_net_forward(sqdet_net_t* net, const void* image_input, void* preds, sqdet_stream_t stream);
/* Binds (NULL: unbinds) a float32 [batch, gh*gw*anchors_per_grid] device buffer: every following sqdet_net_forward also
 * writes interpret_output's det_probs there, from the ConvDet launch's epilogue (see sqdet_convdet_fwd).
 * SQDET_EUNSUPPORTED when the plan's last layer has no score epilogue (sqdet_net_scores_supported). */
int sqdet_net_set_scores(sqdet_net_t* net, float* scores);
int sqdet_net_scores_supported(const sqdet_net_t* net);
/* Serving-loop hook: every following sqdet_net_forward records `hip_event` (a hipEvent_t; NULL: none) on its stream right
 * before the launch of layer `layer_index` -- side work of the PREVIOUS batch (its filter launch, the copy of its rows) that
 * waits for the event on another stream then runs beside the launches behind that point instead of beside the stem.
 * sqdet_net_overlap_layer: the index where side work is cheapest -- the first fire_chain launch (those launches occupy 240
 * of the 256 CUs at batch 32) -- or -1 when the plan has none. */
int sqdet_net_set_signal(sqdet_net_t* net, int layer_index, void* hip_event);
int sqdet_net_overlap_layer(const sqdet_net_t* net);
/* Serving loop without a second stream: the decode + filter of the PREVIOUS batch (what sqdet_detect_filter_scored would
 * launch: same arguments, identical outputs) is handed to the plan and rides in the NEXT sqdet_net_forward as extra "rider"
 * workgroups of its fire_chain launches -- those occupy 240 of the 256 CUs at batch 32, a rider takes an idle CU and one
 * image.  No side stream, no events, no extra launches: stream order alone orders the previous batch's preds / scores
 * (written by its ConvDet launch) before the riders and the riders before the next overwrite.  The out_* rows may be
 * pinned host memory (device-accessible): the rows then need no copy either.  One-shot (consumed by the next forward;
 * preds == NULL cancels).  SQDET_EUNSUPPORTED when the plan cannot carry n images (sqdet_net_rider_capacity: the idle CUs
 * summed over its fire_chain launches; 0 for plans without such launches) -- run sqdet_detect_filter_scored instead. */
int sqdet_net_set_post_job(sqdet_net_t* net, const void* preds, const float* scores, const float* anchors, float* out_boxes,
                           float* out_probs, int32_t* out_cls, int32_t* out_index, int32_t* out_count, int n, int gh, int gw,
                           int apg, int classes, float img_w, float img_h, float exp_thresh, int top_n, int max_out,
                           double nms_thresh, int dtype);
int sqdet_net_rider_capacity(const sqdet_net_t* net);

/* Layer table for measurement: name, 2*MAC flops and algorithmic bytes (every
 * tensor touched once) of each launch of sqdet_net_forward. */
int sqdet_net_num_layers(const sqdet_net_t* net);
int sqdet_net_layer_info(const sqdet_net_t* net, int index, char* name, size_t name_cap, double* flops,
                         double* bytes);
/* 1 when the launcher of layer `index` takes it at the plan's batch and map size under the current options, else 0 (host
 * only).  Every layer of a created plan is launchable: the fused launches address tensors with 32-bit offsets and decline
 * one of 2^31 bytes or more, and plan creation asks the launchers' own predicates, so such a layer is planned unfused. */
int sqdet_net_layer_launchable(const sqdet_net_t* net, int index);
/* Same as sqdet_net_forward but brackets every launch with HIP events on
 * `stream` and, after synchronising, writes per-launch milliseconds to
 * host_ms[num_layers]. */
int sqdet_net_forward_timed(sqdet_net_t* net, const void* image_input, void* preds, float* host_ms,
                            sqdet_stream_t stream);

/* Live measurement inside the normal forward: after sqdet_net_set_probe(net, i, cap) every
 * sqdet_net_forward records a HIP event pair around layer i's launch on the launch stream
 * (up to cap records); sqdet_net_read_probe synchronises those events, returns the per-launch
 * milliseconds and resets the record count.  layer_index -1 disables the probe. */
int sqdet_net_set_probe(sqdet_net_t* net, int layer_index, int max_records);
int sqdet_net_read_probe(sqdet_net_t* net, float* host_ms, int capacity, int* count);

/* ------------------------------------------------------- training labels --
 * Replaces the per-image Python of imdb.read_batch (dataset/imdb.py:195-239: every ground-truth box, in order,
 * claims the free anchor of highest IoU, or the nearest free anchor when nothing overlaps) and the dense
 * placeholder build of train.py:163-224 (sparse_to_dense).  anchors_f64: [num_anchors,4] float64 =
 * mc.ANCHOR_BOX; gt_boxes_f64: [batch,max_objects,4] (cx,cy,w,h, already scaled to the network input);
 * gt_classes / gt_counts: int32 [batch,max_objects] / [batch].  Outputs (all device, float32, fully
 * written): input_mask [batch,A], box_delta_input / box_input [batch,A,4], labels [batch,A,classes];
 * anchor_index int32 [batch,max_objects] (-1 beyond gt_counts). */
int sqdet_build_labels(const double* anchors_f64, const double* gt_boxes_f64, const int* gt_classes,
                       const int* gt_counts, float* input_mask, float* box_delta_input, float* box_input, float* labels,
                       int* anchor_index, int batch, int num_anchors, int max_objects, int classes,
                       sqdet_stream_t stream);

/* sqdet_build_labels_opt: OURS -- more than one positive anchor per object (squeezedet_amd/csrc/assign.hip).  Every box keeps
 * the anchor sqdet_build_labels gives it (anchor_index and that anchor's rows are bit for bit sqdet_build_labels'); the anchors
 * no box claimed are then offered to the boxes by one of two rules, per image, boxes i < gt_counts[b] (clipped to [0, max_objects]):
 *   mode 1 (iou)   anchor a is eligible for box i iff iou(i,a) > 0, iou(i,a) >= iou_thresh and a is among the first max_per_box
 *                  of box i's anchors with iou > 0 in the order larger IoU, ties -> higher index (taken over all anchors, claimed
 *                  ones included): at most max_per_box + 1 positives per box; iou_thresh 0 is a plain top-K;
 *   mode 2 (atss)  candidates: per shape s (anchor a has shape a % anchors_per_grid) the topk anchors of smallest
 *                  d = (gx-ax)*(gx-ax) + (gy-ay)*(gy-ay), ties -> lower index, all of them if the shape has fewer; mean = the
 *                  candidates' IoUs summed in ascending anchor index / their number, var = sum of (iou-mean)*(iou-mean) in the
 *                  same order / their number; a candidate is eligible iff iou > 0, e = iou - mean >= 0 and e*e >= var, and its
 *                  centre lies strictly inside the box (gx - 0.5*gw < ax < gx + 0.5*gw, likewise in y).
 * An unclaimed anchor eligible for several boxes goes to the box of largest IoU, ties -> the lower box index.  iou(i,a) is the
 * float64 expression of util.batch_iou, as in sqdet_build_labels.  Every positive anchor gets sqdet_build_labels' rows (mask 1,
 * the float64 delta rounded once, the box, the one-hot class if 0 <= class < classes); everything else is 0.
 * Further outputs (device int32, fully written): assigned_box [batch,num_anchors] the box index or -1; positives
 * [batch,max_objects] the number of positives per box, 0 behind the image's count.  workspace: device scratch of
 * sqdet_build_labels_opt_workspace_bytes(...) bytes (0: bad arguments), 8-byte aligned; anchors_f64 16-byte aligned.
 * Five launches (sqdet_build_labels' three and two more), no memset node, no synchronisation: capturable in a hipGraph.
 * opt NULL, a mode other than 1 / 2, iou_thresh not >= 0, max_per_box / topk < 1, num_anchors % anchors_per_grid != 0 or any
 * argument sqdet_build_labels refuses: SQDET_EINVAL (its limits: SQDET_EUNSUPPORTED); max_per_box > 64, topk > 32 or
 * anchors_per_grid * min(topk, num_anchors / anchors_per_grid) > 1024: SQDET_EUNSUPPORTED.  Nothing is launched on either. */
enum { SQDET_ASSIGN_IOU = 1, SQDET_ASSIGN_ATSS = 2 };
typedef struct { int mode; double iou_thresh; int max_per_box; int topk; } sqdet_assign_options_t;
size_t sqdet_build_labels_opt_workspace_bytes(int batch, int num_anchors, int max_objects, int anchors_per_grid,
                                              const sqdet_assign_options_t* opt);
int sqdet_build_labels_opt(const double* anchors_f64, const double* gt_boxes_f64, const int* gt_classes, const int* gt_counts,
                           float* input_mask, float* box_delta_input, float* box_input, float* labels, int* anchor_index,
                           int* assigned_box, int* positives, void* workspace, int batch, int num_anchors, int max_objects,
                           int classes, int anchors_per_grid, const sqdet_assign_options_t* opt, sqdet_stream_t stream);

/* --------------------------------------------------------- anchor shapes --
 * OURS for the fitting: the reference ships fixed anchor shapes (config/kitti_squeezeDet_config.py:45-79, the nine k-means
 * shapes of KITTI's objects) and no way to get them for another dataset.
 *
 * sqdet_anchor_kmeans: Lloyd's k-means over box shapes under the IoU distance, `restarts` independent runs at once.
 * The distance of two shapes is 1 - IoU of the two boxes on a common centre, in double, in exactly this order:
 *   inter = min(w, cw) * min(h, ch);   iou = inter / (w*h + cw*ch - inter)
 * wh: device double [n,2] (w, h; finite and > 0 -- the caller checks, squeezedet_amd.anchors does).  centroids: device double
 * [restarts,k,2], the initial centroids on entry, the final ones on exit.  Iteration it = 0 .. max_iter - 1: every box goes
 * to the centroid of highest IoU (the lowest index on a tie, np.argmax); then every centroid becomes the arithmetic mean of
 * its members' (w, h) -- sum over count, in double -- and one without members keeps its value.  Outputs (device, per restart):
 *   assign   int32  [restarts,n]  the assignment of the last iteration
 *   counts   int32  [restarts,k]  its member counts
 *   mean_iou double [restarts]    mean over the boxes of IoU(box, final centroid of assign[box])
 *   iters    int32  [restarts]    the first iteration (counted from 0) whose assignment changed no box, max_iter if none did
 * All max_iter iterations are enqueued -- past convergence one reproduces the fixed point bit for bit -- so nothing returns to
 * the host inside the loop and the call does not synchronise.  Every floating-point sum has a fixed order that depends on n
 * alone (per-workgroup partials in `workspace`, no float atomics): two calls on the same input are bitwise equal.
 * workspace: sqdet_anchor_kmeans_workspace_bytes(n, k, restarts) bytes of device scratch, 8-byte aligned (0: bad arguments).
 * n < 1, k < 1, restarts < 1, max_iter < 1 or a null pointer: SQDET_EINVAL; k > SQDET_ANCHOR_KMEANS_MAX_K or restarts >
 * SQDET_ANCHOR_KMEANS_MAX_RESTARTS: SQDET_EUNSUPPORTED; nothing is launched and no output touched on either. */
enum { SQDET_ANCHOR_KMEANS_MAX_K = 64, SQDET_ANCHOR_KMEANS_MAX_RESTARTS = 64 };
size_t sqdet_anchor_kmeans_workspace_bytes(int n, int k, int restarts);
int sqdet_anchor_kmeans(const double* wh, double* centroids, int* assign, int* counts, double* mean_iou, int* iters,
                        void* workspace, int n, int k, int restarts, int max_iter, sqdet_stream_t stream);

/* sqdet_anchor_coverage: how the anchor grid covers a set of ground-truth boxes.  Replaces the IoU statistics of the
 * mc.DEBUG_MODE branch of imdb.read_batch (dataset/imdb.py:135-139, 203-215, 241-246), per object: from claimed_iou the
 * caller gets its max / min / avg iou and its count of objects with 0 iou.  anchors_f64 [num_anchors,4] = mc.ANCHOR_BOX;
 * gt_boxes_f64 [batch,max_objects,4] and gt_counts [batch] in sqdet_build_labels' padded layout; anchor_index int32
 * [batch,max_objects] as sqdet_build_labels writes it, or NULL.  Outputs (device, [batch,max_objects], fully written):
 *   best_iou    double  the maximum over all anchors of util.batch_iou's expression (utils/util.py:42-54) in double, in the
 *                       reference's operation order
 *   best_index  int32   the first anchor that attains it (np.argmax; 0 when nothing overlaps)
 *   claimed_iou double  the IoU with anchor anchor_index[b,i]; 0 where anchor_index is NULL, -1 or out of range
 * Entries at or beyond gt_counts[b] get 0 / -1 / 0.  One workgroup per entry, one reduction over the anchors (any count).
 * Asynchronous.  batch * max_objects > 2^31 - 1: SQDET_EUNSUPPORTED. */
int sqdet_anchor_coverage(const double* anchors_f64, const double* gt_boxes_f64, const int* gt_counts, const int* anchor_index,
                          double* best_iou, int* best_index, double* claimed_iou, int batch, int num_anchors, int max_objects,
                          sqdet_stream_t stream);

/* -------------------------------------------------------- pre-processing --
 * Replaces the caller-side image preparation of demo.py:186-190 / imdb.py:101-118:
 *   im = cv2.imread(f).astype(float32); im = cv2.resize(im, (dst_w, dst_h)); input = im - BGR_MEANS
 * src_bgr_u8: device uint8 [n,src_h,src_w,3] (BGR, as cv2.imread delivers) -> dst [n,dst_h,dst_w,3] in
 * dtype storage, ready to be image_input.  Bilinear with cv2 INTER_LINEAR coordinates, float32. */
int sqdet_preprocess_bgr(const uint8_t* src_bgr_u8, void* dst, int n, int src_h, int src_w, int dst_h, int dst_w,
                         float mean_b, float mean_g, float mean_r, int dtype, sqdet_stream_t stream);

/* Training-time image preparation of imdb.read_batch (dataset/imdb.py:141-186), the reference's order: per image i
 *   im = float32(u8) - BGR_MEANS      (the means in double: (float)((double)v - mean), rounded once, as NumPy's
 *                                      `im -= mc.BGR_MEANS` with a float64 BGR_MEANS)
 *   D[y, x] = im[y + dy, x + dx] inside im, 0.0f outside, D is (src_h - dy) x (src_w - dx)   (the drift)
 *   flip: D[y, x] = D[y, W' - 1 - x]  (W' = src_w - dx)
 *   dst[i] = cv2.resize(D, (dst_w, dst_h))   (INTER_LINEAR, float32, coordinates as sqdet_preprocess_bgr)
 * src: device uint8, src_bytes long; image i is a BGR [src_h, src_w, 3] array at byte src_offsets[i] (device int64 [n]);
 * geom: device int32 [n,5] = (src_h, src_w, dx, dy, flip) per image; dst [n,dst_h,dst_w,3] in dtype storage.
 * geom and src_offsets are on the device, so THIS CALL CANNOT VALIDATE THEM: the caller must reject (before the call)
 * dx >= src_w, dy >= src_h, |dx| or |dy| > 65535, flip not 0/1 and an image that ends past src_bytes (ops.augment_bgr
 * does).  An image that breaks these rules anyway is left unwritten; no load ever leaves [src, src + src_bytes). */
int sqdet_augment_bgr(const uint8_t* src, size_t src_bytes, const int64_t* src_offsets, const int32_t* geom, void* dst, int n,
                      int dst_h, int dst_w, double mean_b, double mean_g, double mean_r, int dtype, sqdet_stream_t stream);

/* sqdet_augment_bgr with a free WINDOW in place of the drift and an optional colour matrix: per image i, in this order
 *   colour (only when color != NULL): the bytes (b, g, r) of every source pixel as float32,
 *     c_k = ((M[k][0]*b + M[k][1]*g) + M[k][2]*r) + M[k][3];  c_k = fminf(fmaxf(c_k, 0.f), 255.f)   (M = color[i], row-major 3x4)
 *   mean:   v_k = (float)((double)c_k - mean_k)
 *   window: D[y, x] = v[y + y0, x + x0] inside the image, exactly 0.0f outside; D is ch x cw.  The window may lie inside the
 *           image (a crop), contain it (zoom-out onto a canvas of the mean colour) or straddle it; neither the matrix nor its
 *           offset touches the padding
 *   flip:   D[y, x] = D[y, cw - 1 - x]
 *   dst[i] = cv2.resize(D, (dst_w, dst_h)) as sqdet_augment_bgr: the bilinear taps clamp at the WINDOW's border, so a crop never
 *           uses an image pixel outside its window
 * geom: device int32 [n,7] = (src_h, src_w, x0, y0, cw, ch, flip); color: device float32 [n,12] or NULL; the rest as
 * sqdet_augment_bgr.  The window (dx, dy, src_w - dx, src_h - dy) with color == NULL gives sqdet_augment_bgr's output bit for bit.
 * As there, THIS CALL CANNOT VALIDATE geom: the caller must reject |x0| or |y0| > 65535, cw or ch outside [1, 65535] (a larger
 * cw is valid only where x0 + cw == src_w, a larger ch only where y0 + ch == src_h: the window of a drift sqdet_augment_bgr accepts),
 * flip not 0/1 and an image that ends past src_bytes (ops.augment_bgr_window does).  An image that breaks these rules anyway is left unwritten;
 * no load ever leaves [src, src + src_bytes). */
int sqdet_augment_bgr_window(const uint8_t* src, size_t src_bytes, const int64_t* src_offsets, const int32_t* geom,
                             const float* color, void* dst, int n, int dst_h, int dst_w, double mean_b, double mean_g,
                             double mean_r, int dtype, sqdet_stream_t stream);

/* The mosaic: FOUR source images per output image, each in its own pane.  Output image i is cut at column xc = split[i][0] and
 * row yc = split[i][1] (device int32 [n,2], 0 <= xc <= dst_w, 0 <= yc <= dst_h) into
 *   pane 0 = rows [0, yc) x columns [0, xc)        pane 1 = rows [0, yc) x columns [xc, dst_w)
 *   pane 2 = rows [yc, dst_h) x columns [0, xc)    pane 3 = rows [yc, dst_h) x columns [xc, dst_w)
 * and pane p, ph x pw pixels, holds cv2.resize(D_p, (pw, ph)), where D_p is exactly the window D that sqdet_augment_bgr_window
 * builds -- colour, mean in double rounded once, window with 0.0f outside the image, mirror, in this order -- for the source image
 * at byte part_offsets[i][p] (device int64 [n,4]) with geom[i][p] = (src_h, src_w, x0, y0, cw, ch, flip) (device int32 [n,4,7]) and
 * the matrix color[i][p] (device float32 [n,4,12], or NULL: no matrix).  The resize coordinates are those of (cw, ch) -> (pw, ph)
 * and the taps clamp at the window's border: nothing is blended across a seam, a pane never uses a pixel of another pane's source.
 * A pane without pixels (xc = 0 or dst_w, yc = 0 or dst_h) is never examined: its offset, geometry and matrix may hold anything, and
 * split = (dst_w, dst_h) gives sqdet_augment_bgr_window's output for part 0 bit for bit.  dst [n,dst_h,dst_w,3] in dtype storage;
 * float16 is the float32 value converted once.
 * As above, THIS CALL CANNOT VALIDATE split, geom or part_offsets: the caller must reject a split outside [0, dst_w] x [0, dst_h] and,
 * for every pane that has pixels, whatever sqdet_augment_bgr_window's caller must reject for an image (ops.augment_bgr_mosaic
 * does).  A pane with pixels that breaks the rules anyway is left unwritten while the image's other panes are written; an image
 * whose split is out of range is left unwritten; no load ever leaves [src, src + src_bytes). */
int sqdet_augment_bgr_mosaic(const uint8_t* src, size_t src_bytes, const int64_t* part_offsets, const int32_t* geom,
                             const int32_t* split, const float* color, void* dst, int n, int dst_h, int dst_w, double mean_b,
                             double mean_g, double mean_r, int dtype, sqdet_stream_t stream);

/* -------------------------------------------------------- detection table --
 * What the KITTI, the Pascal VOC and the COCO-style evaluation below score: ONE layout, filled by sqdet_kitti_ingest /
 * sqdet_voc_ingest with the values of the respective dataset's detection files, by sqdet_coco_ingest with unrounded x,y,w,h
 * (or by the caller).  Caller-owned, device; `cap` rows per image
 * (<= SQDET_KITTI_MAX_DETECTIONS = SQDET_VOC_MAX_DETECTIONS = SQDET_COCO_MAX_DETECTIONS), num_images images:
 *   det_box double [num_images,cap,4] (x1,y1,x2,y2; COCO: x,y,w,h), det_score double [num_images,cap], det_cls int32 [num_images,cap]
 *   (0 <= class < the dataset's class count), det_count int32 [num_images] (rows of the image, class-major; zero it to
 *   reset), status int32 [2] (a rejected ingest, sticky; zero it to reset).
 *
 * ------------------------------------------------------- KITTI evaluation --
 * Replaces the scoring half of src/eval.py (:69-101) -- the detection files of dataset/kitti.py:100-127, the KITTI C++
 * evaluator's 2D box metric (dataset/kitti-eval/cpp/evaluate_object.cpp) and kitti.analyze_detections (:182-296) -- with
 * device tables.  All values are double: exactly what the evaluator reads back from the files the reference writes.
 *
 * Detection table: see above; det_cls 0 car, 1 pedestrian, 2 cyclist.
 * Ground truth (device): image i owns rows [gt_offsets[i], gt_offsets[i+1]) (<= SQDET_KITTI_MAX_GROUNDTRUTH), gt_box double
 *   [G,4] (x1,y1,x2,y2), gt_truncation double [G], gt_occlusion int32 [G], gt_type int32 [G] (SQDET_KITTI_* type codes). */
enum { SQDET_KITTI_MAX_DETECTIONS = 512, SQDET_KITTI_MAX_GROUNDTRUTH = 128, SQDET_KITTI_ANALYSIS_COUNTERS = 8 };
enum { SQDET_KITTI_CAR = 0, SQDET_KITTI_PEDESTRIAN = 1, SQDET_KITTI_CYCLIST = 2, SQDET_KITTI_VAN = 3, SQDET_KITTI_PERSON_SITTING = 4,
       SQDET_KITTI_DONTCARE = 5, SQDET_KITTI_OTHER = 6 };
enum { SQDET_KITTI_ERR_LOC = 0, SQDET_KITTI_ERR_CLS = 1, SQDET_KITTI_ERR_BG = 2, SQDET_KITTI_ERR_MISSED = 3 };

/* Appends n images of filter rows (sqdet_filter_prediction layout: boxes float32 [n,max_out,4] cx,cy,w,h, probs float32
 * [n,max_out], cls int32 [n,max_out], count int32 [n]) as table images [image_offset, image_offset + n).  Per row, in double:
 * cx,w /= x_scale and cy,h /= y_scale (scales: double [n,2], NULL = 1), bbox_transform, then x1,y1,x2,y2 rounded as '%.2f'
 * and the score as '%.3f' print them (half-to-even on the exact value), read back as the nearest double.  Rows are stored
 * class-major, filter order within a class: the order of the files.  The counts live on the device: a count outside
 * [0, max_out] or a class outside 0..2 makes the WHOLE call write nothing and marks status; sqdet_kitti_evaluate then
 * returns SQDET_EINVAL.  max_out > cap: SQDET_EUNSUPPORTED.  Asynchronous. */
int sqdet_kitti_ingest(const float* boxes, const float* probs, const int32_t* cls, const int32_t* count, const double* scales,
                       int n, int max_out, double* det_box, double* det_score, int32_t* det_cls, int32_t* det_count,
                       int32_t* status, int image_offset, int num_images, int cap, sqdet_stream_t stream);

/* Scores the table (the evaluator's cleanData / computeStatistics / getThresholds / eval_class, MIN_OVERLAP 0.7/0.5/0.5):
 * host_precision double [9,41] (row = class * 3 + difficulty: easy, moderate, hard; precision after the running maximum),
 * host_ap double [9] (mean of precision[0,4,..,40]), host_evaluated int32 [3] (the class was detected at least once: the
 * evaluator writes its files only then).  workspace: sqdet_kitti_eval_workspace_bytes(num_gt) of device scratch.
 * SYNCHRONISES `stream` once, at the end; the host outputs are untouched on failure.  An image over the row limits:
 * SQDET_EUNSUPPORTED; a rejected ingest in the table: SQDET_EINVAL. */
size_t sqdet_kitti_eval_workspace_bytes(int num_gt);
int sqdet_kitti_evaluate(const double* det_box, const double* det_score, const int32_t* det_cls, const int32_t* det_count,
                         const int32_t* status, int num_images, int cap, const int32_t* gt_offsets, const double* gt_box,
                         const double* gt_truncation, const int32_t* gt_occlusion, const int32_t* gt_type, int num_gt,
                         void* workspace, double* host_precision, double* host_ap, int32_t* host_evaluated, sqdet_stream_t stream);

/* kitti.analyze_detections on the table: per image the detections by descending score (stable), the first len(rois) of
 * them matched by batch_iou against the image's ground-truth rois (roi_offsets as gt_offsets; roi_box double [R,4] cx,cy,w,h
 * as bbox_transform_inv gives them, roi_cls int32 [R]).  counters int32 [SQDET_KITTI_ANALYSIS_COUNTERS + 1]: detections,
 * objects, correct, localisation, classification, background, repeated, detected objects, then an over-limit flag.
 * Records of det_error_file.txt: image i writes rec_count[i] rows from row 2 * roi_offsets[i]: rec_type (SQDET_KITTI_ERR_*),
 * rec_cls, rec_box double [.,4] (cx,cy,w,h), rec_score (-1 for a missed object); capacity 2R rows.  Asynchronous. */
int sqdet_kitti_analyze(const double* det_box, const double* det_score, const int32_t* det_cls, const int32_t* det_count,
                        int num_images, int cap, const int32_t* roi_offsets, const double* roi_box, const int32_t* roi_cls,
                        int num_rois, int32_t* counters, int32_t* rec_count, int32_t* rec_type, int32_t* rec_cls,
                        double* rec_box, double* rec_score, sqdet_stream_t stream);

/* -------------------------------------------------- Pascal VOC evaluation --
 * Replaces the scoring half of the reference for Pascal VOC -- the per-class detection files of
 * dataset/pascal_voc.py:98-109 and the VOC AP metric of dataset/voc_eval.py:33-64,124-204 -- with device tables, for every
 * class at once.  All values are double: exactly what voc_eval reads back with float() from the files the reference writes.
 *
 * Detection table: see above; det_box 1-based as the files carry them, det_cls 0 <= class < classes <= SQDET_VOC_MAX_CLASSES.
 * Ground truth (device): image i owns rows [gt_offsets[i], gt_offsets[i+1]) (<= SQDET_VOC_MAX_GROUNDTRUTH), gt_box double
 *   [G,4] (the XML's integers xmin,ymin,xmax,ymax), gt_cls int32 [G] (-1: a name outside the class list, never matched),
 *   gt_difficult int32 [G].
 *
 * TIE RULE (ours): the rows of a class are ordered by descending score, equal scores by image index, then by row index
 * within the image.  The reference's np.argsort(-confidence) (voc_eval.py:151) is not stable, so its order of equal
 * scores is unspecified; this one is fixed, and two runs on the same table give bitwise the same results. */
enum { SQDET_VOC_MAX_DETECTIONS = 512, SQDET_VOC_MAX_GROUNDTRUTH = 128, SQDET_VOC_MAX_CLASSES = 64 };

/* pascal_voc.evaluate_detections' file writer (pascal_voc.py:98-109) into the table: appends n images of filter rows
 * (sqdet_filter_prediction layout, as sqdet_kitti_ingest) as table images [image_offset, image_offset + n).  Per row, in
 * float32 as the reference's NumPy does: cx,w /= (float)x_scale and cy,h /= (float)y_scale (scales: double [n,2], NULL = no
 * division; eval.py:83-84), bbox_transform (cx - w/2, ...; eval.py:91), + 1 (pascal_voc.py:107-108); then each coordinate
 * is the double nearest to what '{:.1f}' prints for it and the score the double nearest to its '{:.3f}'.  Rows are stored
 * class-major, filter order within a class: the order of the per-class files.  A count outside [0, max_out] or a class
 * outside [0, classes) makes the WHOLE call write nothing and marks status; sqdet_voc_evaluate then returns SQDET_EINVAL.
 * max_out > cap: SQDET_EUNSUPPORTED.  Asynchronous. */
int sqdet_voc_ingest(const float* boxes, const float* probs, const int32_t* cls, const int32_t* count, const double* scales,
                     int n, int max_out, int classes, double* det_box, double* det_score, int32_t* det_cls, int32_t* det_count,
                     int32_t* status, int image_offset, int num_images, int cap, sqdet_stream_t stream);

/* voc_eval (voc_eval.py:124-204) and voc_ap (:33-64) for every class, on the device: per (image, class) the class's
 * detections by descending score are matched greedily to the image's objects of the class ('+1' overlaps, ovmax > 0.5 in
 * double, np.argmax's first index; a difficult best match counts as neither, a taken one as false positive, :187-195); the
 * flags are put in the class's order (TIE RULE above), summed by a prefix sum, rec = tp / npos and
 * prec = tp / max(tp + fp, DBL_EPSILON); then both APs.
 * Host outputs, each [classes]: host_ap07 (the 11-point form, thresholds i * 0.1, `ap + p / 11.` in threshold order:
 * bitwise the reference's), host_ap_area (area under the precision envelope; the terms are summed in a fixed order that is
 * not NumPy's pairwise one, so it may differ from the reference by n * 2^-53 for n rows), host_npos (non-difficult
 * objects), host_num_det (rows).  A class without rows has AP 0 (:147-148).  curve_cls >= 0: that class's rec and prec
 * (host_num_det[curve_cls] values each, the class's order) into the device buffers curve_rec / curve_prec of
 * num_images * cap doubles; curve_cls < 0: they may be NULL.  workspace: sqdet_voc_eval_workspace_bytes(num_images, cap,
 * classes) of device scratch.  SYNCHRONISES `stream` once, at the end; the host outputs are untouched on failure.  An image
 * over the row limits: SQDET_EUNSUPPORTED; a rejected ingest in the table: SQDET_EINVAL. */
size_t sqdet_voc_eval_workspace_bytes(int num_images, int cap, int classes);
int sqdet_voc_evaluate(const double* det_box, const double* det_score, const int32_t* det_cls, const int32_t* det_count,
                       const int32_t* status, int num_images, int cap, int classes, const int32_t* gt_offsets,
                       const double* gt_box, const int32_t* gt_cls, const int32_t* gt_difficult, int num_gt, void* workspace,
                       double* host_ap07, double* host_ap_area, int32_t* host_npos, int32_t* host_num_det, int curve_cls,
                       double* curve_rec, double* curve_prec, sqdet_stream_t stream);

/* ---------------------------------------------------- COCO-style evaluation --
 * The published COCOeval bbox protocol on the detection table: average precision over a list of IoU thresholds (0.50:0.05:0.95),
 * by object area, and average recall at a list of detection limits (1 / 10 / 100), for every class at once.  It has no
 * counterpart in the reference; it scores the same tables as the two evaluators above with a metric that moves when boxes
 * get tighter or looser.  All values are double.
 *
 * Detection table: see above; det_box holds (x, y, w, h) -- the top-left corner and the size, as COCO results files carry them.
 * Ground truth (device): image i owns rows [gt_offsets[i], gt_offsets[i+1]) (<= SQDET_COCO_MAX_GROUNDTRUTH), gt_box double
 *   [G,4] (x, y, w, h), gt_cls int32 [G] (outside [0, classes): never matched, never counted), gt_area double [G],
 *   gt_ignore int32 [G]: bit 0 = ignore, bit 1 = iscrowd.
 *
 * TIE RULE: the rows of a class are ordered by descending score, equal scores by image index, then by rank in the image
 * (where equal scores keep the row order).  That is the order a stable sort gives the per-image lists put one after
 * another, which is what COCOeval does (mergesort), so the rule is the protocol's own. */
enum { SQDET_COCO_MAX_DETECTIONS = 512, SQDET_COCO_MAX_GROUNDTRUTH = 128, SQDET_COCO_MAX_CLASSES = 128,
       SQDET_COCO_MAX_IOU_THRESHOLDS = 10, SQDET_COCO_MAX_RECALL_THRESHOLDS = 128, SQDET_COCO_MAX_AREA_RANGES = 4,
       SQDET_COCO_MAX_DET_LIMITS = 3, SQDET_COCO_MAX_KEPT = 128 };

/* A results file's rows into the table (step "load results"): appends n images of filter rows (sqdet_filter_prediction
 * layout, as sqdet_kitti_ingest) as table images [image_offset, image_offset + n).  Per row, in double: cx,w /= x_scale and
 * cy,h /= y_scale (scales: double [n,2], NULL = 1), then (cx - w/2, cy - h/2, w, h); the score is the float32 widened.
 * Nothing is rounded and nothing is added.  Rows are stored class-major, filter order within a class.  A count outside
 * [0, max_out] or a class outside [0, classes) makes the WHOLE call write nothing and marks status; sqdet_coco_evaluate then
 * returns SQDET_EINVAL.  max_out > cap or classes > SQDET_COCO_MAX_CLASSES: SQDET_EUNSUPPORTED.  Asynchronous. */
int sqdet_coco_ingest(const float* boxes, const float* probs, const int32_t* cls, const int32_t* count, const double* scales,
                      int n, int max_out, int classes, double* det_box, double* det_score, int32_t* det_cls, int32_t* det_count,
                      int32_t* status, int image_offset, int num_images, int cap, sqdet_stream_t stream);

/* COCOeval's evaluateImg and accumulate for every (class, area range, detection limit, IoU threshold), on the device.
 * Host inputs, used as they are (np.linspace's values; nothing is recomputed on the device): iou_thrs double [num_iou],
 * rec_thrs double [num_rec], area_ranges double [num_area,2] (lo, hi, both inclusive), max_dets int32 [num_max_dets]
 * (positive, ascending).
 * Step "IoU": iw = min(dx+dw, gx+gw) - max(dx, gx), ih likewise; 0 unless both are positive; else iw*ih over
 *   dw*dh + gw*gh - iw*ih, or over dw*dh for a crowd.
 * Step "evaluateImg", per (image, class): the class's rows by descending score (stable), the first max_dets[last] kept; an
 *   object is ignored in an area range by its ignore or crowd bit or an area outside the range; per threshold t the rows in
 *   rank order each take, with best = min(t, 1 - 1e-10), the object of largest IoU >= best among the non-ignored ones not yet
 *   taken at t, the later one of equals -- and only if there is none, likewise among the ignored ones (a crowd can be taken
 *   again).  A matched row is ignored when its object is, an unmatched one when its own w*h lies outside the range.
 * Step "accumulate", per (class, area range a, limit m, threshold t): the rows of rank < max_dets[m] in the class's order
 *   (TIE RULE), tp = matched & !ignored, fp = !matched & !ignored, integer prefix sums, rc = tp / npig,
 *   pr = tp / (fp + tp + 2.220446049250313e-16), pr's suffix maximum, recall = rc[last] (0 without rows), and
 *   precision[r] = pr at the first row with rc >= rec_thrs[r] (0 past the end).  npig (the class's non-ignored objects in
 *   the range) == 0 leaves the whole entry at -1.
 * Device outputs, the per-row results in the class's order (class c's rows start at the sum of host_num_det[< c]):
 *   row_rank int32 [num_images * cap] (the row's rank in its image) and row_word int32 [num_area, num_images * cap] (bit t:
 *   matched at threshold t; bit num_iou + t: ignored at it).
 * Host outputs: host_precision double [num_iou, num_rec, classes, num_area, num_max_dets], host_recall double [num_iou,
 *   classes, num_area, num_max_dets], host_npig int32 [classes, num_area], host_num_det int32 [classes] (kept rows).
 * workspace: sqdet_coco_eval_workspace_bytes(num_images, cap, classes) of device scratch (sized for the largest lists).
 * One stream; SYNCHRONISES it once, at the end; the host outputs are untouched on failure.  Over a limit above (or an image
 * over the row limits): SQDET_EUNSUPPORTED; a rejected ingest in the table: SQDET_EINVAL. */
size_t sqdet_coco_eval_workspace_bytes(int num_images, int cap, int classes);
int sqdet_coco_evaluate(const double* det_box, const double* det_score, const int32_t* det_cls, const int32_t* det_count,
                        const int32_t* status, int num_images, int cap, int classes, const int32_t* gt_offsets,
                        const double* gt_box, const int32_t* gt_cls, const double* gt_area, const int32_t* gt_ignore, int num_gt,
                        const double* iou_thrs, int num_iou, const double* rec_thrs, int num_rec, const double* area_ranges,
                        int num_area, const int32_t* max_dets, int num_max_dets, void* workspace, int32_t* row_rank,
                        int32_t* row_word, double* host_precision, double* host_recall, int32_t* host_npig, int32_t* host_num_det,
                        sqdet_stream_t stream);

/* ------------------------------------------------------ training summaries --
 * Replaces the per-tensor summary ops of the training graph: tf.summary.histogram of every trainable variable and of its
 * gradient (nn_skeleton.py:353-358) and _activation_summary (nn_skeleton.py:736-755: histogram, tf.nn.zero_fraction,
 * reduce_mean, reduce_max, reduce_min of a layer's output) -- for MANY segments of ONE buffer in one call, so a whole flat
 * parameter or gradient bucket of the trainers is one launch (plus a one-workgroup-per-segment finishing launch).
 *
 * base: device, dtype storage (SQDET_F32 / SQDET_F16), base_count elements long; segment s is elements
 * [offsets[s], offsets[s] + counts[s]) of it (device int64 [n_segments]; any element-aligned start, any count incl. 0 and 1;
 * nothing outside a segment is read -- the 64-element padding of the flat buckets is not counted).  Every element is widened
 * to float32 first.  edges: device float32 [n_bins + 1], ascending (1 <= n_bins <= 1024); binning is by float32 comparison
 * only, so the integer fields equal the counts of np.searchsorted(edges, x, side="right") exactly.
 * records: device, n_segments records of sqdet_tensor_stats_record_bytes(n_bins) bytes (8-byte aligned):
 *   int64 count        the segment's element count (-1: the segment does not lie inside [0, base_count) and was not read)
 *   int64 nonfinite    NaN or +-inf elements
 *   int64 zeros        elements equal to 0 (-0.0 included): tf.nn.zero_fraction * count
 *   float min, max     over the finite elements; +inf / -inf when there is none
 *   double sum, sumsq  over the finite elements, accumulated in float64
 *   int64 under, hist[n_bins], over    finite x < edges[0]; edges[i] <= x < edges[i+1]; x >= edges[n_bins]
 * sum and sumsq are reduced in a fixed order (per-workgroup partials in `workspace`, then one ordered pass; no float atomics):
 * two calls on the same data, device and segment table give bitwise the same records.  workspace:
 * sqdet_tensor_stats_workspace_bytes(n_segments, n_bins) bytes of device scratch, 8-byte aligned.  The call zeroes what it
 * accumulates into on `stream`, allocates nothing and does not synchronise. */
size_t sqdet_tensor_stats_record_bytes(int n_bins);
size_t sqdet_tensor_stats_workspace_bytes(int n_segments, int n_bins);
int sqdet_tensor_stats_many(const void* base, int64_t base_count, const int64_t* offsets_dev, const int64_t* counts_dev,
                            int n_segments, const float* edges_dev, int n_bins, void* records_dev, void* workspace,
                            int dtype, sqdet_stream_t stream);

/* ------------------------------------------------------------ drawing --
 * Boxes and labels drawn into a batch of images that is already on the device: the reference's _draw_box of the training
 * image summary (src/train.py:51-99), the rectangle + text of imdb.visualize_detections (src/dataset/imdb.py:254-305) and
 * of the demos (src/demo.py), which draw with cv2 / PIL on the host, one image at a time.
 *
 * An ITEM is SQDET_DRAW_ITEM_BYTES (64) bytes:
 *   int32 x0, y0, x1, y1   a rectangle, corners in either order, any value (used clamped to +-2^30)
 *   uint8 b, g, r          its colour, BGR like the images
 *   uint8 anchor           SQDET_DRAW_BOTTOM_LEFT: the label's text cell has its left column at x0 and its bottom row at y1
 *                          (where _draw_box puts its text); SQDET_DRAW_TOP_LEFT: the cell starts at (x0, y0) (visualize_detections)
 *   int32 label_len        0 .. SQDET_DRAW_LABEL_MAX (used clamped to that range)
 *   char  label[32]        bytes; 8 bytes of padding follow
 * An item TABLE is [n, cap] items (16-byte aligned) + int32 counts [n]: image i draws its first clamp(counts[i], 0, cap) rows.
 *
 * sqdet_draw_items: out uint8 [n,h,w,3] = the images with the items of up to SQDET_DRAW_MAX_TABLES tables drawn over them,
 * table after table, row after row (painter's order: a later item overwrites an earlier one; an item is its rectangle, then
 * its label).  ONE launch; every output pixel GATHERS its value from the tables, so the result does not depend on scheduling.
 *   images  in_type SQDET_F32 / SQDET_F16: the network input [n,h,w,3], mean-subtracted BGR; a pixel is restored as
 *           rint(float32(x) + float32(host_bgr_means[c])) (half to even), clamped to [0, 255].  SQDET_DRAW_U8: uint8 BGR
 *           [n,h,w,3], taken as it is (host_bgr_means is not read; out may be the images themselves).
 *   rgb_out 0: out is BGR; 1: out is RGB (channels reversed, colours with them).
 *   rectangle: one pixel wide, the set cv2.rectangle(.., 1) paints -- x in {x0, x1} and min(y0,y1) <= y <= max(y0,y1), or
 *           y in {y0, y1} and min(x0,x1) <= x <= max(x0,x1) -- clipped to the image.
 *   label:  character k occupies the 6x8 cell k cells to the right of the anchor cell; its 5x7 glyph (sqdet_draw_font5x7) sits
 *           in columns 1..5 and rows 0..6 of the cell; set glyph bits take the item's colour, everything else keeps what is
 *           under it.  Bytes outside ASCII 32..126 draw as '?'.  Clipped to the image.
 * item_tables / item_counts / caps: HOST arrays of n_tables device pointers / capacities.  The capacities together may not
 * exceed SQDET_DRAW_MAX_ITEMS (256), nor n*h*w 2^31 - 1: SQDET_EUNSUPPORTED.
 *
 * sqdet_draw_build_items: item rows from box rows, on the device.  boxes [n,rows,4] float32 (boxes_f64 = 0: the out_boxes of
 * sqdet_detect_filter / sqdet_filter_prediction) or float64 (1: a ground-truth table); cls int32 [n,rows]; counts int32 [n]
 * (used clamped to [0, rows]); probs float32 [n,rows] or NULL.  Image i keeps, in order, its rows j < counts[i] with
 * double(probs[i,j]) > plot_thresh (all of them when probs is NULL; the reference compares a float32 with a Python float,
 * i.e. in double) and writes them to items [n,cap]; item_counts[i] = their number.
 *   coordinates  diagonal = 0: int() -- truncation toward zero -- of cx - w/2, cy - h/2, cx + w/2, cy + h/2 (util.bbox_transform)
 *           computed in the boxes' own precision; diagonal = 1: int() of the four values as they are.  NaN -> 0.
 *   colour  class_bgr (device uint8 [classes,3], the reference's cdict) where it is given and the class is in range, else
 *           (b, g, r).
 *   label   names: device bytes [classes, SQDET_DRAW_NAME_BYTES], NUL-padded ('?' for a class out of range).  label_format
 *           SQDET_DRAW_LABEL_NAME: "<name>"; _NAME_COLON_PROB: "<name>: (%.2f)"; _NAME_PROB: "<name> (%.2f)" of
 *           double(float32 prob) with the digits Python's '%' prints (|prob| >= 1e7: "?.??"); cut at SQDET_DRAW_LABEL_MAX bytes.
 * rows > cap or cap > SQDET_DRAW_MAX_ITEMS: SQDET_EUNSUPPORTED.  Both calls are asynchronous, allocate nothing and validate
 * their arguments before they touch the device.
 *
 * sqdet_draw_font5x7: the font, 95 glyphs (ASCII 32..126) x 7 rows, one byte per row, bit 4 = leftmost column, into
 * host_out (capacity >= 665 bytes).  The table is this project's own (csrc/font5x7.h). */
enum { SQDET_DRAW_U8 = 2 };
enum { SQDET_DRAW_BOTTOM_LEFT = 0, SQDET_DRAW_TOP_LEFT = 1 };
enum { SQDET_DRAW_LABEL_NAME = 0, SQDET_DRAW_LABEL_NAME_COLON_PROB = 1, SQDET_DRAW_LABEL_NAME_PROB = 2 };
#define SQDET_DRAW_ITEM_BYTES 64
#define SQDET_DRAW_MAX_ITEMS 256
#define SQDET_DRAW_MAX_TABLES 4
#define SQDET_DRAW_LABEL_MAX 31
#define SQDET_DRAW_NAME_BYTES 32
int sqdet_draw_items(const void* images, unsigned char* out, int in_type, int n, int h, int w, const float* host_bgr_means,
                     int rgb_out, const void* const* item_tables, const int32_t* const* item_counts, const int* caps,
                     int n_tables, sqdet_stream_t stream);
int sqdet_draw_build_items(const void* boxes, int boxes_f64, const float* probs, const int32_t* cls, const int32_t* counts,
                           int n, int rows, int diagonal, double plot_thresh, const unsigned char* names, int classes,
                           const unsigned char* class_bgr, int b, int g, int r, int label_format, int anchor, void* items,
                           int32_t* item_counts, int cap, sqdet_stream_t stream);
int sqdet_draw_font5x7(unsigned char* host_out, size_t capacity);

/* ------------------------------------------------------------ tracking --
 * Object identities across the frames of a video or of a bank of cameras: tracking-by-detection over the rows that
 * sqdet_detect_filter* / sqdet_filter_prediction emit (out_boxes float32 [n,rows,4] (cx,cy,w,h), out_probs float32 [n,rows],
 * out_cls int32 [n,rows], out_count int32 [n]).  The reference has no counterpart: this stage is the project's own, placed
 * behind the filter so that the rows never go back to the host.  All arithmetic is float64, every operator below ONE IEEE
 * operation in the order written (csrc/track.hip is built without contraction), so a sequential NumPy restatement
 * (tests/track_reference.py) agrees with the tables and outputs bit for bit.
 *
 * There are S independent STREAMS, each with SQDET_TRACK_CAP (64) track slots.  A call processes n = S*F images: image s*F + f
 * is frame f of stream s, and a stream's F frames are processed in order (a video: S = 1, F = batch; a camera bank: S = batch,
 * F = 1).  rows <= 64, else SQDET_EUNSUPPORTED.
 *
 * State per slot: for each coordinate c of (cx, cy, w, h) a constant-velocity filter, x[c] = (p, v) and P[c] = (pp, pv, vv);
 * int32 cls, id, state (0 free, 1 tentative, 2 confirmed), hits, miss, age; float32 score.  Per stream: int32 next_id (1 after
 * a reset) and dropped.  A reset is: every table zero, next_id one.  A freed slot keeps its other fields as they were.
 *
 * One frame of one stream -- slots and rows are always visited in ascending index:
 *  1. count = clamp(out_count, 0, rows) (the filter reports an overflow as a negative count).
 *  2. Predict every live slot (state != 0): h = max(x[h].p, 1.0); qp = (w_pos*h)*(w_pos*h); qv = (w_vel*h)*(w_vel*h); per
 *     coordinate p = p + v, pp' = ((pp + pv) + (pv + vv)) + qp, pv' = pv + vv, vv' = vv + qv; age += 1.  The predicted box is
 *     (p_cx, p_cy, max(p_w, 1.0), max(p_h, 1.0)).
 *  3. Valid rows: d < count, the four box values and the prob finite, w > 0 and h > 0.  An invalid row takes part in nothing.
 *     High rows: double(prob) > high_thresh.  Low rows: low_thresh < double(prob) <= high_thresh.
 *  4. Affinity M[t,d] of a live slot t and a valid row d of the same class: the IoU of the predicted box (1) and the row's box
 *     widened to double (2) in the expression of the reference's util.iou (utils/util.py:9-30):
 *     lr = min(cx1 + 0.5*w1, cx2 + 0.5*w2) - max(cx1 - 0.5*w1, cx2 - 0.5*w2), tb likewise; both > 0: inter = lr*tb,
 *     M = inter / (w1*h1 + w2*h2 - inter); else 0.  Another class: 0.  (min(a, b) is b < a ? b : a, max(a, b) is b > a ? b : a.)
 *  5. Greedy association of a set of slots and a set of rows: repeatedly take the free pair with the largest M -- ties go to
 *     the lower slot, then the lower row -- and stop when no free pair has M >= iou_thresh.  Stage one: all live slots x high
 *     rows.  Stage two: the still unmatched CONFIRMED slots x low rows.
 *  6. Update every matched slot, with h = max(x[h].p, 1.0) after the predict and r = (w_pos*h)*(w_pos*h); per coordinate, z the
 *     row's value: y = z - p; s = pp + r; kp = pp / s; kv = pv / s; p = p + kp*y; v = v + kv*y; pp' = pp - kp*pp;
 *     pv' = pv - kp*pv; vv' = vv - kv*pv.  hits += 1, miss = 0, score = prob; a tentative slot becomes confirmed when
 *     hits >= min_hits.  det_track_id[d] = id, det_track_state[d] = state.
 *  7. Every unmatched live slot: miss += 1; it is freed if it was tentative or if miss > max_age.
 *  8. Every unmatched high row, in row order, takes the lowest free slot (one freed in step 7 included): x[c] = (z, 0),
 *     P[c] = (a*a, 0, b*b) with h = max(z_h, 1.0), a = (2*w_pos)*h, b = (10*w_vel)*h; cls and score from the row;
 *     id = next_id++, hits = 1, miss = 0, age = 1; tentative, or confirmed when min_hits <= 1.  The row gets the new id and
 *     state.  No free slot: dropped += 1 and the row gets nothing.
 *  9. Every row j < rows that got nothing -- invalid, unmatched low, dropped, j >= count -- has det_track_id -1 and
 *     det_track_state 0.
 *
 * sqdet_track_update: ONE launch, asynchronous on `stream`, allocates nothing, validates its arguments before it touches the
 * device.  tables: HOST struct of device pointers, the caller's: x float64 [S,64,4,2], P float64 [S,64,4,3], cls / id /
 * state / hits / miss / age int32 [S,64], score float32 [S,64], next_id / dropped int32 [S].  params: HOST struct;
 * iou_thresh > 0, thresholds and weights finite, min_hits and max_age >= 0.  Outputs det_track_id, det_track_state int32
 * [n,rows].  Stream s is walked by one workgroup; max_workgroups > 0: the S streams are walked by at most that many workgroups
 * (<= 0: one per stream), as sqdet_detect_filter_scored does.
 *
 * sqdet_track_build_items: draw items (sqdet_draw_items) from detection rows and the two outputs.  Image i keeps, in order,
 * its rows j < clamp(counts[i], 0, rows) with det_track_state == 2, det_track_id > 0 and double(prob) > plot_thresh.
 * Coordinates as sqdet_draw_build_items with float32 boxes and diagonal = 0; the label is "<name> #<id>" ('?' for a class
 * out of range), cut at SQDET_DRAW_LABEL_MAX bytes; the colour is palette[id % palette_len], palette a device uint8
 * [palette_len,3] (BGR).  rows > cap or cap > SQDET_DRAW_MAX_ITEMS: SQDET_EUNSUPPORTED. */
#define SQDET_TRACK_CAP 64
typedef struct sqdet_track_tables {
  double* x;
  double* P;
  int32_t* cls;
  int32_t* id;
  int32_t* state;
  int32_t* hits;
  int32_t* miss;
  int32_t* age;
  float* score;
  int32_t* next_id;
  int32_t* dropped;
} sqdet_track_tables_t;
typedef struct sqdet_track_params {
  double iou_thresh;      /* 0.3 */
  double high_thresh;     /* 0.5 */
  double low_thresh;      /* 0.1 */
  double w_pos;           /* 1/20 */
  double w_vel;           /* 1/160 */
  int32_t min_hits;       /* 3 */
  int32_t max_age;        /* 30 */
} sqdet_track_params_t;
int sqdet_track_update(const sqdet_track_tables_t* tables, const float* boxes, const float* probs, const int32_t* cls,
                       const int32_t* counts, int streams, int frames, int rows, const sqdet_track_params_t* params,
                       int32_t* det_track_id, int32_t* det_track_state, int max_workgroups, sqdet_stream_t stream);
int sqdet_track_build_items(const float* boxes, const float* probs, const int32_t* cls, const int32_t* counts,
                            const int32_t* det_track_id, const int32_t* det_track_state, int n, int rows, double plot_thresh,
                            const unsigned char* names, int classes, const unsigned char* palette, int palette_len, int anchor,
                            void* items, int32_t* item_counts, int cap, sqdet_stream_t stream);

/* ------------------------------------------------- tracking evaluation --
 * The published CLEAR-MOT counts (MOTA, MOTP, identity switches, fragmentations, mostly tracked / mostly lost) and IDF1 of the
 * tracker's outputs against labelled objects, on the device and straight from sqdet_track_update's arrays, so that identities
 * never return to the host.  The reference has no tracker and no tracking metric: this stage is the project's own, and THIS TEXT
 * is its definition (tests/mot_reference.py restates it sequentially in NumPy; csrc/mot_eval.hip is built without contraction
 * and agrees with it bit for bit in every counter, in iou_sum and in every table).
 *
 * Layout as the tracker's: S independent streams, a call takes n = S*F images, image s*F + f is frame f of stream s; state
 * persists across calls until a reset (every table zero).
 *
 * Hypotheses are the tracker's arrays: boxes float32 [n,rows,4] (cx,cy,w,h), cls int32 [n,rows], counts int32 [n],
 * det_track_id and det_track_state int32 [n,rows]; rows <= SQDET_MOT_CAP (64).  Row j is a hypothesis when
 * j < clamp(count, 0, rows), state == 2, id > 0, the four box values are finite, w > 0 and h > 0, 0 <= cls < classes, and no
 * lower row of the frame that passes these tests carries the same id.  Ground truth: gt_box float64 [n,G,4] (cx,cy,w,h), gt_id
 * int32 [n,G] (> 0), gt_cls, gt_flags int32 [n,G] (bit 0: IGNORE -- KITTI DontCare, a MOT distractor or conf 0), gt_count int32
 * [n]; G <= 64; row j is an object by the same rule without the state.  classes <= SQDET_MOT_MAX_CLASSES (128).
 *
 * One frame of one stream.  "In order" is ascending row index.  All floating arithmetic is float64 (a hypothesis box is widened,
 * exactly), one IEEE operation per operator.  A stream whose status word is not zero skips the frame altogether.
 *  5. (first, because it can stop the stream) Identities get DENSE INDICES in order of first appearance: the frame's non-ignored
 *     objects in order, then its hypotheses in order.  A stream holds at most SQDET_MOT_MAX_OBJECTS (256) object identities and
 *     SQDET_MOT_MAX_HYPOTHESES (1024) hypothesis identities; obj_id / obj_cls and hyp_id / hyp_cls record an identity's id and
 *     the class of its first appearance.  If the frame's new identities do not all fit, the stream's status word gets
 *     SQDET_MOT_STATUS_OBJECTS and / or SQDET_MOT_STATUS_HYPOTHESES and NOTHING else changes, in this frame or a later one.
 *     An ignored object has no identity.
 *  1. IoU of every (object, hypothesis) pair of the same class in the expression of the tracker's step 4 (box 1 the object, box 2
 *     the hypothesis); another class: 0.  A pair is ALLOWED when IoU >= iou_thresh (inclusive; 0 < iou_thresh <= 1).  Its integer
 *     cost is q = (int64) floor((1.0 - IoU) * 1048576.0).
 *  2. Continuity (CLEAR-MOT; the rule of py-motmetrics).  For each non-ignored object in order whose `last` -- the hypothesis id
 *     it was most recently matched to, however long ago -- is the id of a hypothesis of this frame that is still free and allowed
 *     with it: the pair is matched and both ends leave the pool.
 *  3. Optimal assignment of the remaining objects (ignored ones included) and the remaining hypotheses, each compacted in order
 *     to rows i and columns j: a square matrix of side N = max(rows, columns) with cost q for an allowed pair and BIG = 2^32 for a
 *     pair that is not allowed and for a padding cell, solved by assign() below; a pair assigned at BIG is unmatched.  (64 * 2^20
 *     < BIG: the optimum first maximises the number of matches, then minimises the summed q, exactly, in integers.)  With no
 *     remaining object or no remaining hypothesis nothing is assigned.
 *  4. Counts, per class (counts int64 [S,classes,5]: tp, fn, fp, idsw, ignored_hyp; iou_sum float64 [S,classes]).  A hypothesis
 *     matched to an ignored object is DROPPED from everything: ignored_hyp += 1.  A matched non-ignored object: tp += 1;
 *     iou_sum = iou_sum + IoU (objects in order); idsw += 1 when it has a `last` that differs from the hypothesis id; then
 *     last = that id.  An unmatched non-ignored object: fn += 1 (it keeps its `last`).  An unmatched hypothesis: fp += 1.  Per
 *     object identity: obj_present += 1; matched: obj_tracked += 1, obj_frag += 1 when obj_run == 2, obj_run = 1; unmatched:
 *     obj_run 1 becomes 2 (obj_run: 0 never matched, 1 matched at its previous present frame, 2 matched before but not at its
 *     previous present frame).  Per hypothesis identity that was not dropped: hyp_frames += 1.  For every allowed pair of a
 *     non-ignored object and a hypothesis that was not dropped, matched or not: overlap[g][t] += 1 at their dense indices.
 *
 * assign(cost[R][C]), R <= C, int64 -> the row of every column, -1 for a free one.  The shortest-augmenting-path Hungarian method
 * with integer potentials u[R], v[C] (zero at first).  Rows are inserted in ascending order.  Inserting row i: minv[j] = 2^62,
 * way[j] = -1, no column scanned; i0 = i, j0 = -1; then rounds: column j0 (if any) becomes scanned; for every unscanned column j,
 * cur = cost[i0][j] - u[i0] - v[j], and cur < minv[j] sets minv[j] = cur, way[j] = j0; j1 is the unscanned column of smallest
 * minv, the LOWEST index among equals, and delta its minv; every scanned column j: u[row of j] += delta, v[j] -= delta; every
 * unscanned one: minv[j] -= delta; u[i] += delta; j0 = j1; a free j0 ends the rounds, otherwise i0 = the row of j0.  Then the
 * path is flipped: while j0 >= 0: w = way[j0]; the row of j0 becomes the row of w (row i when w < 0); j0 = w.  Optimal
 * assignments are not unique and MOTP depends on the pairs: the kernels return THESE pairs, not merely this cost.
 *
 * sqdet_mot_evaluate, per stream with G_ids object and T_ids hypothesis identities: IDF1's global matching is assign() on the
 * G_ids x max(T_ids, G_ids) matrix of cost -overlap[g][t] (columns past T_ids are zero); idtp[c] is the sum of overlap over the
 * assigned pairs whose object identity has class c, idfn[c] the sum of obj_present of that class minus idtp[c], idfp[c] the sum of
 * hyp_frames of the hypothesis identities of class c minus idtp[c].  An object identity is mostly tracked when 5*tracked >=
 * 4*present, mostly lost when 5*tracked < present, partly tracked otherwise.  Output per stream and class, SQDET_MOT_COUNTERS
 * (14) int64 words: tp, fn, fp, idsw, ignored_hyp, frag, mt, pt, ml, idtp, idfn, idfp, gt_ids, hyp_ids; and iou_sum.  The caller
 * derives MOTA = 1 - (fn + fp + idsw) / (tp + fn), MOTP = iou_sum / tp, IDF1 = 2 idtp / (2 idtp + idfp + idfn), precision and
 * recall, and sums counters over streams and classes for an overall line.
 *
 * sqdet_mot_update: ONE launch, asynchronous on `stream`, allocates nothing, validates its arguments before it touches the
 * device; one wave walks a stream; max_workgroups as sqdet_track_update.  tables: HOST struct of device pointers, the caller's:
 * obj_id / obj_cls / obj_last / obj_present / obj_tracked / obj_frag / obj_run int32 [S,256], hyp_id / hyp_cls / hyp_frames int32
 * [S,1024], n_obj / n_hyp / status int32 [S], counts int64 [S,classes,5], iou_sum float64 [S,classes], overlap int32
 * [S,256,1024].  sqdet_mot_evaluate: one workgroup per stream; result_device: int64 [S,classes,14] device words it may
 * overwrite; it synchronises `stream` ONCE and then fills host_counters int64 [S,classes,14] and host_iou_sum float64
 * [S,classes].  A stream with a status word set: SQDET_EUNSUPPORTED, and -- as on every failure -- the host outputs are untouched.
 * It changes no table: updates may go on after it.  Both use plain vector loads and stores only, and no atomics. */
#define SQDET_MOT_CAP 64
#define SQDET_MOT_MAX_OBJECTS 256
#define SQDET_MOT_MAX_HYPOTHESES 1024
#define SQDET_MOT_MAX_CLASSES 128
#define SQDET_MOT_COUNTERS 14
#define SQDET_MOT_STATUS_OBJECTS 1
#define SQDET_MOT_STATUS_HYPOTHESES 2
typedef struct sqdet_mot_tables {
  int32_t* obj_id;
  int32_t* obj_cls;
  int32_t* obj_last;
  int32_t* obj_present;
  int32_t* obj_tracked;
  int32_t* obj_frag;
  int32_t* obj_run;
  int32_t* hyp_id;
  int32_t* hyp_cls;
  int32_t* hyp_frames;
  int32_t* n_obj;
  int32_t* n_hyp;
  int32_t* status;
  int64_t* counts;
  double* iou_sum;
  int32_t* overlap;
} sqdet_mot_tables_t;
int sqdet_mot_update(const sqdet_mot_tables_t* tables, const float* boxes, const int32_t* cls, const int32_t* counts,
                     const int32_t* det_track_id, const int32_t* det_track_state, const double* gt_box, const int32_t* gt_id,
                     const int32_t* gt_cls, const int32_t* gt_flags, const int32_t* gt_count, int streams, int frames, int rows,
                     int gt_rows, int classes, double iou_thresh, int max_workgroups, sqdet_stream_t stream);
int sqdet_mot_evaluate(const sqdet_mot_tables_t* tables, int streams, int classes, int64_t* result_device, int64_t* host_counters,
                       double* host_iou_sum, sqdet_stream_t stream);

/* ------------------------------------------------------------ utilities --
 * Device -> pinned-host copy issued as a KERNEL: dst is host memory mapped into the device's address space
 * (hipHostMalloc); nbytes a multiple of 16.  Used by the serving loop to hand the <= 64 filtered rows per image
 * (the return value of the reference's filter_prediction, nn_skeleton.py:696-734) to the host without a blocking
 * memcpy call.  The data is complete on the host once `stream` has been synchronised. */
int sqdet_copy_to_mapped_host(const void* src_device, void* dst_pinned_host, size_t nbytes, sqdet_stream_t stream);

/* Hardware self-test used by the GPU test-suite: runs one MFMA of each shape
 * the kernels rely on with index-encoded operands and writes the observed
 * (row, col) of every accumulator register to host_out (see csrc/probe.hip). */
int sqdet_probe_mfma_layout(int32_t* host_out, int capacity);

/* Box calibration (bench.py's `box_mfma_tflops` / `box_copy_gbs`; no reference counterpart -- the reference has no
 * device code).  sqdet_calib_mfma enqueues a fixed MFMA microkernel (512 workgroups x 4 waves x iters x 8 independent
 * 16x16x32 float16 MFMAs; scratch: >= 131072 device floats it may overwrite) and returns the flops it performs in
 * *flops; sqdet_calib_copy enqueues a plain 16-byte-per-lane device copy of `bytes` bytes.  The caller times them with
 * events on `stream`. */
int sqdet_calib_mfma(float* scratch, size_t scratch_floats, int iters, double* flops, sqdet_stream_t stream);
int sqdet_calib_copy(const void* src, void* dst, size_t bytes, sqdet_stream_t stream);
/* The MFMA loop in the shapes that settle what the box's ceiling is: shape 0 = mfma_f32_16x16x32_f16 (8 independent accumulators
 * per wave), shape 1 = mfma_f32_32x32x16_f16 (4 independent accumulators; the instruction the guide's 2495 TF/s was measured
 * with); `waves_per_simd` co-resident 256-thread workgroups per CU (grid = CUs x waves_per_simd, returned in *workgroups);
 * zero_operands != 0: all-zero A / B (power management gives clock back on them).  ticks[2 * wg] = shader cycles (s_memtime),
 * ticks[2 * wg + 1] = 100 MHz ticks (s_memrealtime) of workgroup wg's loop: effective clock = 100 MHz x cycles / ticks,
 * cycles per MFMA = cycles / (iters x accumulators).  scratch >= workgroups x 256 floats, ticks >= workgroups x 2. */
int sqdet_calib_mfma2(float* scratch, size_t scratch_floats, unsigned long long* ticks, size_t ticks_count, int iters, int shape,
                      int waves_per_simd, int zero_operands, double* flops, int* workgroups, sqdet_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SQDET_H */
