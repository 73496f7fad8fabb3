// Fused network stem for gfx950, host side: conv (KSxKS, stride 2, Cin = 3) + bias + ReLU + max-pool 3x3/s2 in ONE launch --
// conv1 + pool1 of SqueezeDet (reference src/nets/squeezeDet.py:40-44: 3x3/s2 SAME + pool SAME), SqueezeDet+
// (src/nets/squeezeDetPlus.py:40-44: 7x7/s2 VALID + pool VALID) and ResNet50 (src/nets/resnet50_convDet.py:41-45: 7x7/s2,
// 64 couts, pool VALID).  Unfused, conv1 writes 188x621x64 and pool1 reads it back -- 36.4 MB of the 133 MB per image
// (fp16); fused, the conv activations never leave the CU.  This file fills StemArgs (stem_args), gates the two persistent
// kernels' shapes (stem_pers_shape) and tries the kernels in order (stem_launch, stem_squeeze_launch):
//   stem4.hip  stem_phase_dma: persistent, lane-local pooling over three column phases; fp16 3x3 / 64 couts, images >= 523 wide
//   stem3.hip  stem_pers: persistent, strip lanes + DPP pooling; the same shapes from 235 wide, or "stem_algo" 3
//   stem5.hip  stem_k7: the float16 7x7 stems (4-channel LDS rows, one K chunk per kernel row, no gather)
//   stem2.hip  stem_strip: pool in registers; every other shape / dtype (float32 training), or "stem_algo" 2
#include "stem.h"

namespace sqdet {

StemArgs stem_args(const void* x, const void* w_packed, const float* bias, void* y, int n, int h, int w, int cout, int k,
                   int conv_pad, int pool_pad, int dtype, int y_cstride, int y_coffset) {
  const ConvGeom g = conv_geom(k, 3, cout, dtype);
  StemArgs a;
  a.x = x; a.wp = w_packed; a.bias = bias; a.y = y;
  a.N = n; a.H = h; a.W = w;
  a.Hc = out_size(h, k, 2, conv_pad); a.Wc = out_size(w, k, 2, conv_pad);
  a.Hp = out_size(a.Hc, 3, 2, pool_pad); a.Wp = out_size(a.Wc, 3, 2, pool_pad);
  a.ptc = pad_before(h, k, 2, conv_pad); a.plc = pad_before(w, k, 2, conv_pad);
  a.ptp = pad_before(a.Hc, 3, 2, pool_pad); a.plp = pad_before(a.Wc, 3, 2, pool_pad);
  a.Cout = cout; a.nchunk = g.nchunk; a.kdim = g.kdim;
  a.tiles_x = a.tiles_y = 0;
  a.y_cstride = y_cstride; a.y_coffset = y_coffset;
  a.ws2 = nullptr; a.bs2 = nullptr; a.s_out = nullptr;
  return a;
}

bool stem_pers_shape(const StemArgs& a, int k, int dtype, int patch_cols, int tile_rows, int tile_cols) {
  if (dtype != SQDET_F16 || k != 3 || a.Cout != 64) return false;
  if (a.W % 2 != 0 || a.plc % 2 != 0 || a.y_cstride % 8 != 0 || a.y_coffset % 8 != 0) return false;
  if ((size_t)a.H * a.W * 6 >= (1ull << 31) || a.W * 6 < 2 * patch_cols * 16) return false;
  if ((size_t)a.N * a.Hp * a.Wp * a.y_cstride * 2 >= (1ull << 31)) return false;
  const long tiles_x = (a.Wp + tile_cols - 1) / tile_cols, tiles_y = (a.Hp + tile_rows - 1) / tile_rows;
  return a.N * tiles_x * tiles_y < (1l << 30);
}

// conv(k, stride 2, Cin 3) + bias + relu + maxpool(3, stride 2).  *handled=false: not eligible (the caller runs conv and pool
// apart; the strip kernel declines channel strides it cannot store with 16-byte vectors).
int stem_launch(const void* x, const void* w_packed, const float* bias, void* y, int n, int h, int w, int cout, int k,
                int conv_pad, int pool_pad, int dtype, int y_cstride, int y_coffset, hipStream_t st, bool* handled) {
  *handled = false;
  if (conv_algo() != 0) return SQDET_OK;
  if (!((k == 3 && cout == 64) || (k == 7 && (cout == 96 || cout == 64)))) return SQDET_OK;   // SqueezeDet, SqueezeDet+, ResNet50
  const ConvGeom g = conv_geom(k, 3, cout, dtype);
  if (!g.gather || g.ngroups != 1) return SQDET_OK;
  const StemArgs a = stem_args(x, w_packed, bias, y, n, h, w, cout, k, conv_pad, pool_pad, dtype, y_cstride, y_coffset);
  if (a.Hp <= 0 || a.Wp <= 0) return SQDET_OK;
  // the first kernel that takes the shape; "stem_algo" 3 keeps to the persistent and the strip kernel, 2 to the strip kernel
  const int algo = tune(TUNE_STEM_ALGO);
  const struct { int (*launch)(StemArgs, int, int, hipStream_t, bool*); bool tried; } order[] = {
      {stem_phase_launch, algo == 0},
      {stem_pers_launch, algo == 0 || algo == 3},
      {stem_k7_launch, algo == 0},
      {stem_strip_launch, true}};
  for (const auto& kern : order) {
    if (!kern.tried) continue;
    const int rc = kern.launch(a, k, dtype, st, handled);
    if (rc != SQDET_OK || *handled) return rc;
  }
  return SQDET_OK;
}

// conv1 + pool1 + the next layer's squeeze1x1 (64 -> 16 couts) in one launch: only the squeeze tensor [n, Hp, Wp, 16] is written
// (persistent fp16 3x3 stems only).  *handled = false: not eligible.
int stem_squeeze_launch(const void* x, const void* w_packed, const float* bias, const void* ws2_packed, const float* bs2,
                        void* s_out, int n, int h, int w, int cout, int k, int conv_pad, int pool_pad, int s2, int dtype,
                        hipStream_t st, bool* handled) {
  *handled = false;
  if (!stem_squeeze_eligible(h, w, cout, k, conv_pad, pool_pad, s2, dtype, n)) return SQDET_OK;
  StemArgs a = stem_args(x, w_packed, bias, nullptr, n, h, w, cout, k, conv_pad, pool_pad, dtype, cout, 0);
  a.ws2 = ws2_packed; a.bs2 = bs2; a.s_out = s_out;
  if (tune(TUNE_STEM_ALGO) == 0) {
    const int rc = stem_phase_launch(a, k, dtype, st, handled);
    if (rc != SQDET_OK || *handled) return rc;
  }
  return stem_pers_launch(a, k, dtype, st, handled);
}

// Gated on stem_pers's tile, not the phase kernel's: stem_pers is the squeeze form's last resort, so its width bound (235) is the
// form's; the phase kernel takes the wider images first.
bool stem_squeeze_eligible(int h, int w, int cout, int k, int conv_pad, int pool_pad, int s2, int dtype, int n) {
  if (conv_algo() != 0 || tune(TUNE_STEM_ALGO) == 2 || k != 3 || cout != 64 || s2 != 16 || dtype != SQDET_F16) return false;
  const ConvGeom gs = conv_geom(1, cout, s2, dtype);   // fire2's squeeze1x1: two K chunks of one tile
  if (gs.gather || gs.nchunk != 2 || gs.nt != 1 || gs.ngroups != 1) return false;
  const StemArgs a = stem_args(nullptr, nullptr, nullptr, nullptr, n, h, w, cout, k, conv_pad, pool_pad, dtype, cout, 0);
  return a.Hp > 0 && a.Wp > 0 && stem_pers_shape(a, k, dtype, QRP, QPR, 4 * QSP);
}

}  // namespace sqdet

extern "C" int sqdet_stem_conv_pool_squeeze_fwd(const void* x, const void* w_packed, const float* bias, const void* w_next_s_packed,
                                                const float* b_next_s, void* sq_out, int n, int h, int w, int cout, int k,
                                                int conv_pad_mode, int pool_pad_mode, int next_s, int dtype, sqdet_stream_t stream) {
  using namespace sqdet;
  SQDET_REQUIRE(x && w_packed && bias && w_next_s_packed && b_next_s && sq_out, "stem_squeeze: null pointer");
  SQDET_REQUIRE(n > 0 && h > 0 && w > 0 && cout > 0 && k > 0 && next_s > 0, "stem_squeeze: bad dims");
  bool handled = false;
  const int rc = stem_squeeze_launch(x, w_packed, bias, w_next_s_packed, b_next_s, sq_out, n, h, w, cout, k, conv_pad_mode,
                                     pool_pad_mode, next_s, dtype, as_stream(stream), &handled);
  if (rc != SQDET_OK) return rc;
  SQDET_UNSUPPORTED(!handled, "stem_squeeze: needs the float16 3x3 / 64-cout stem of even width followed by a 64 -> 16 squeeze1x1");
  return SQDET_OK;
}

extern "C" int sqdet_stem_conv_pool_squeeze_supported(int h, int w, int cout, int k, int conv_pad_mode, int pool_pad_mode,
                                                      int next_s, int dtype, int n) {
  return sqdet::stem_squeeze_eligible(h, w, cout, k, conv_pad_mode, pool_pad_mode, next_s, dtype, n) ? 1 : 0;
}

// C ABI: the fused stem as its own entry point (see include/sqdet.h).
extern "C" int sqdet_stem_conv_pool_fwd(const void* x, const void* w_packed, const float* bias, void* y, int n, int h,
                                        int w, int cout, int k, int conv_pad_mode, int pool_pad_mode, int dtype,
                                        sqdet_stream_t stream) {
  using namespace sqdet;
  SQDET_REQUIRE(x && w_packed && bias && y, "stem: null pointer");
  SQDET_REQUIRE(dtype == SQDET_F16 || dtype == SQDET_F32, "stem: bad dtype");
  SQDET_REQUIRE(n > 0 && h > 0 && w > 0 && cout > 0 && k > 0, "stem: bad dims");
  bool handled = false;
  const int saved = conv_algo();
  SQDET_UNSUPPORTED(saved != 0, "stem: fused kernel disabled by conv_algo=generic");
  int rc = stem_launch(x, w_packed, bias, y, n, h, w, cout, k, conv_pad_mode, pool_pad_mode, dtype, cout, 0,
                       as_stream(stream), &handled);
  if (rc != SQDET_OK) return rc;
  SQDET_UNSUPPORTED(!handled, "stem: only (k=3, cout=64) and (k=7, cout=96 or 64) stems are fused");
  return SQDET_OK;
}
