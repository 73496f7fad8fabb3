// Host-side launchers, eligibility predicates and tuning knobs that one source file defines and another calls: the ONE
// declaration of each (default arguments included).  Every file that defines one of them includes this header (directly or
// through conv_common.h), so a changed signature is a compile error, not a second overload.  Declarations only, no device
// code.  The launchers that take a kernel family's own argument struct stay beside it: stem.h, chain.h, postproc.h,
// conv3x3_tile.h.
#pragma once
#include "common.h"

namespace sqdet {

struct ConvArgs;  // conv_common.h

// ---- conv.hip
// Which kernel family conv2d_launch may pick: 0 = auto (fast paths when eligible),
// 1 = generic only (conv_direct / conv_gather).  Set from SQDET_CONV_ALGO=generic (tests, A/B).
int conv_algo();
// experiment knobs set through sqdet_set_option (0 = built-in heuristic)
// fire_fuse: 0 / 1 = a fire module is one fused launch wherever a fused kernel takes it (the default since round 5), 2 = never,
// 10 = the round-1..4 rule (only maps of <= 100 k pixels)
// stem_algo (0, 2 or 3; sqdet_set_option rejects anything else): 0 = the first eligible of phase kernel (stem4.hip), persistent strip-lane
// kernel (stem3.hip), 7x7 kernel (stem5.hip), strip kernel (stem2.hip); 3 = persistent, then strip kernel only; 2 = strip kernel only
// conv_pool: 1 (the default) = a 3x3 conv followed by a 2x2/s2 SAME max-pool is one launch of conv3x3_tile's POOL2 form wherever it
// takes the shape (plans and sqdet_conv2d_maxpool2_*), 0 = never
// g1_wr / g1_mbw / g1_ntw: conv1x1_pipe's wave layout (waves along the pixel blocks: 1, 2, 4), pixel blocks per wave (2, 4, 8) and cout tiles per wave -- tools/g1_sweep.py
enum { TUNE_C1_WAVES = 0, TUNE_C1_MT = 1, TUNE_C1_MIN_TILES = 2, TUNE_FIRE_FUSE = 3, TUNE_STEM_ALGO = 4, TUNE_DBG = 5, TUNE_G1_WR = 6, TUNE_G1_MBW = 7, TUNE_G1_NTW = 8, TUNE_G1_NS = 9,
       TUNE_CONV_POOL = 10 };
int tune(int which);
int conv2d_launch(const void* x, const void* w_packed, const float* bias, void* y, int n, int h, int w, int cin,
                  int cout, int k, int stride, int pad_mode, int relu, int dtype, int y_cstride, int y_coffset,
                  hipStream_t st);
int conv2d_launch_ex(const void* x, const void* w_packed, const float* bias, void* y, int n, int h, int w, int cin,
                     int cout, int k, int stride, int pad_mode, int relu, int dtype, int y_cstride, int y_coffset,
                     int x_cstride, int x_coffset, int accum, hipStream_t st);
int conv2d_launch_masked(const void* x, const void* w_packed, const float* bias, void* y, int n, int h, int w, int cin,
                         int cout, int k, int stride, int pad_mode, int relu, int dtype, int y_cstride, int y_coffset,
                         int x_cstride, int x_coffset, int accum, const void* relu_of, hipStream_t st);
// ConvDet + scores in one launch (sqdet_convdet_fwd); convdet.hip: the score epilogue's shapes
int convdet_scored_launch(const void* x, const void* w_packed, const float* bias, void* preds, float* scores, int n, int h, int w,
                          int cin, int apg, int classes, int dtype, hipStream_t st);
bool convdet_score_supported(int cout, int apg, int classes, int dtype);

// ---- the fast paths conv.hip's dispatch tries (*handled = false: not this kernel's shape)
int conv1x1_stream_launch(const ConvArgs& a, const ConvGeom& g, int dtype, hipStream_t st, bool* handled);
int conv1x1_tile_launch(const ConvArgs& a, const ConvGeom& g, int dtype, hipStream_t st, bool* handled);   // gemm1x1.hip
int conv1x1_deepk_launch(const ConvArgs& a, const ConvGeom& g, int dtype, hipStream_t st, bool* handled);  // conv1x1k.hip
int conv3x3_tile_launch(const ConvArgs& a, const ConvGeom& g, int dtype, hipStream_t st, bool* handled);
// conv3x3.hip: the same with max_pool 2x2/s2/SAME in the epilogue (y = the pooled tensor); dry = eligibility only
int conv3x3_pool2_launch(const ConvArgs& a, const ConvGeom& g, int dtype, hipStream_t st, bool* handled, bool dry,
                         unsigned char* widx = nullptr);
bool conv2d_maxpool2_eligible(int n, int h, int w, int cin, int cout, int dtype);
int conv2d_maxpool2_launch(const void* x, const void* w_packed, const float* bias, void* y, int n, int h, int w, int cin, int cout,
                           int relu, int dtype, hipStream_t st, unsigned char* widx = nullptr);
// conv3x3.hip: both expands of a fire module from ONE staged squeeze tile (the tile kernel's PAIR form)
bool conv3x3_pair_eligible(int n, int h, int w, int s, int e1, int e3, int dtype);
int conv3x3_pair_launch(const void* sq_in, const void* w3, const float* b3, const void* w1, const float* b1, void* y, int n, int h, int w,
                        int s, int e1, int e3, int dtype, hipStream_t st, bool* handled);

// ---- pool.hip, bn.hip
int maxpool_launch(const void* x, void* y, int n, int h, int w, int c, int k, int stride, int pad_mode, int dtype,
                   hipStream_t st);
int fold_bn_launch(const float* w, const float* cbias, const float* gamma, const float* beta, const float* mean,
                   const float* var, float eps, float* wf, float* bf, int k, int cin, int cout, hipStream_t st);

// ---- stem.hip: conv1 + pool1 in one launch (+ the first fire module's squeeze1x1)
int stem_launch(const void* x, const void* w_packed, const float* bias, void* y, int n, int h, int w, int cout, int k,
                int conv_pad, int pool_pad, int dtype, int y_cstride, int y_coffset, hipStream_t st, bool* handled);
int stem_squeeze_launch(const void* x, const void* w_packed, const float* bias, const void* ws2_packed, const float* bs2,
                        void* s_out, int n, int h, int w, int cout, int k, int conv_pad, int pool_pad, int s2, int dtype,
                        hipStream_t st, bool* handled);
bool stem_squeeze_eligible(int h, int w, int cout, int k, int conv_pad, int pool_pad, int s2, int dtype, int n);

// ---- fire.hip: a fire module in one launch (the *_keep forms also write the module's squeeze tensor: training)
// Two predicates per fused fire launch.  *_eligible: the channel shape and dtype alone (the *_supported probes, weight packing).
// *_eligible_at: the same AND the sizes of a launch on n images of h x w -- every tensor the kernel addresses with 32-bit buffer
// offsets below 2^31 bytes, the tile counter in range.  The launcher declines exactly where its *_eligible_at is false, and the
// planner (net.cpp) asks the same function with the plan's batch, so a plan never holds a launch that will decline by size.
bool fire_fused_eligible(int cin, int s, int e1, int e3, int dtype);
bool fire_fused_eligible_at(int n, int h, int w, int cin, int s, int e1, int e3, int dtype);
int fire_fused_launch(const void* x, const void* ws, const float* bs, const void* w1, const float* b1, const void* w3,
                      const float* b3, void* y, int n, int h, int w, int cin, int s, int e1, int e3, int dtype,
                      hipStream_t st, bool* handled);
int fire_fused_launch_keep(const void* x, const void* ws, const float* bs, const void* w1, const float* b1, const void* w3,
                           const float* b3, void* sq_out, void* y, int n, int h, int w, int cin, int s, int e1, int e3, int dtype,
                           hipStream_t st, bool* handled);

// ---- fire2.hip: persistent streaming fused fire for the large, few-channel modules
bool fire_stream_eligible(int cin, int s, int e1, int e3, int dtype);
bool fire_stream_eligible_at(int n, int h, int w, int cin, int s, int e1, int e3, int dtype, int pool);
int fire_stream_launch_keep(const void* x, const void* ws, const float* bs, const void* w1, const float* b1, const void* w3,
                            const float* b3, void* sq_out, void* y, int n, int h, int w, int cin, int s, int e1, int e3, int dtype,
                            hipStream_t st, bool* handled);
int fire_stream_launch(const void* x, const void* ws, const float* bs, const void* w1, const float* b1, const void* w3,
                       const float* b3, void* y, int n, int h, int w, int cin, int s, int e1, int e3, int dtype,
                       hipStream_t st, bool* handled);
// pool != 0: fire module + max_pool 3x3/s2/SAME in one launch; y is the pooled tensor
int fire_stream_launch_ex(const void* x, const void* ws, const float* bs, const void* w1, const float* b1, const void* w3,
                          const float* b3, void* y, int n, int h, int w, int cin, int s, int e1, int e3, int dtype,
                          int pool, hipStream_t st, bool* handled);
// the expand half of a fire module from its squeeze tensor (+ the 3x3/s2 SAME max-pool behind it when pool != 0)
bool fire_expand_stream_eligible(int s, int e1, int e3, int dtype);
bool fire_expand_stream_eligible_at(int n, int h, int w, int s, int e1, int e3, int dtype, int pool);
int fire_expand_stream_launch(const void* sq_in, const void* w1, const float* b1, const void* w3, const float* b3, void* y,
                              int n, int h, int w, int s, int e1, int e3, int dtype, int pool, hipStream_t st, bool* handled);
// whole fire module from x, its concat tensor replaced by the NEXT module's squeeze tensor (fire2 / fire4 of SqueezeDet)
bool fire_squeeze_next_eligible(int cin, int s, int e1, int e3, int s2, int dtype);
bool fire_squeeze_next_eligible_at(int n, int h, int w, int cin, int s, int e1, int e3, int s2, int dtype);
int fire_squeeze_next_launch(const void* x, const void* ws, const float* bs, const void* w1, const float* b1, const void* w3,
                             const float* b3, const void* ws2, const float* bs2, void* s_out, int n, int h, int w, int cin,
                             int s, int e1, int e3, int s2, int dtype, hipStream_t st, bool* handled);
bool fire_expand_squeeze_next_eligible(int s, int e1, int e3, int s2, int pool, int dtype);
bool fire_expand_squeeze_next_eligible_at(int n, int h, int w, int s, int e1, int e3, int s2, int pool, int dtype);
int fire_expand_squeeze_next_launch(const void* sq_in, const void* w1, const float* b1, const void* w3, const float* b3,
                                    const void* ws2, const float* bs2, void* s_out, int n, int h, int w, int s, int e1, int e3,
                                    int s2, int pool, int dtype, hipStream_t st, bool* handled);
// fire3.hip: the same launch as a DMA-fed kernel sized for four waves per SIMD (SqueezeDet's four shapes)
int fire_dma_launch(const void* sq_in, const void* w1, const float* b1, const void* w3, const float* b3, const void* ws2,
                    const float* bs2, void* s_out, int n, int h, int w, int s, int e1, int e3, int s2, int pool, int dtype,
                    hipStream_t st, bool* handled);

// ---- chain.hip (its launchers: chain.h)
bool fire_chain_eligible(int s, int e1, int e3, int s2, int dtype);
bool fire_chain_eligible_at(int n, int h, int w, int s, int e1, int e3, int s2, int dtype);

}  // namespace sqdet
