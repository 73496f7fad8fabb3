// The fused-stem kernels' shared arguments and launchers: stem2.hip (strip kernel, pool in registers), stem3.hip (persistent,
// strip lanes), stem4.hip (persistent, phase form with LDS-DMA) and stem5.hip (7x7 stems).  stem.hip is their host side: it fills
// StemArgs, holds the shape gate of the two persistent kernels and tries the kernels in order.
#pragma once
#include "conv_common.h"

namespace sqdet {

struct StemArgs {
  const void* x;
  const void* wp;
  const float* bias;
  void* y;
  int N, H, W;          // input
  int Hc, Wc;           // conv output
  int Hp, Wp;           // pooled output
  int ptc, plc;         // conv pad before (top, left)
  int ptp, plp;         // pool pad before
  int Cout, nchunk, kdim;
  int tiles_x, tiles_y;
  int y_cstride, y_coffset;
  // stem3.hip, squeeze form: the pooled pixels are not stored; the NEXT layer's squeeze1x1 (64 -> S2 = 16 couts: fire2's) runs on
  // them in registers and only that tensor [n, Hp, Wp, 16] is written
  const void* ws2;      // packed squeeze kernel (standard fragment order, 2 K-chunks x 1 tile), NULL = plain stem
  const float* bs2;
  void* s_out;
};

// Fills everything but tiles_x / tiles_y (each kernel's launcher sets its own) and the squeeze form's three pointers (NULL).
StemArgs stem_args(const void* x, const void* w_packed, const float* bias, void* y, int n, int h, int w, int cout, int k,
                   int conv_pad, int pool_pad, int dtype, int y_cstride, int y_coffset);

// The fp16 3x3 / 64-cout stem the persistent kernels (stem3.hip, stem4.hip) take: even W and even left pad (dword-aligned patch
// rows), 16-byte aligned channel slices, one image and the output below 2 GiB (32-bit buffer offsets), an image at least two
// patches wide (patch_cols = 16-byte pieces fetched per patch row) and fewer than 2^30 tiles of tile_rows x tile_cols pooled pixels.
bool stem_pers_shape(const StemArgs& a, int k, int dtype, int patch_cols, int tile_rows, int tile_cols);
// stem3.hip's tile, here because stem_squeeze_eligible gates on it
constexpr int QPR = 4;                    // pooled rows per tile
constexpr int QSP = 7;                    // pooled columns per wave strip
constexpr int QRP = 44;                   // 16-byte pieces fetched per row (704 B >= 117 * 3 * 2)

int stem_strip_launch(StemArgs a, int k, int dtype, hipStream_t st, bool* handled);
int stem_pers_launch(StemArgs a, int k, int dtype, hipStream_t st, bool* handled);   // stem3.hip: fp16, 3x3, 64 couts
int stem_phase_launch(StemArgs a, int k, int dtype, hipStream_t st, bool* handled);  // stem4.hip: the same shapes, images >= 523 wide
int stem_k7_launch(StemArgs a, int k, int dtype, hipStream_t st, bool* handled);     // stem5.hip: fp16 7x7 stems (SqueezeDet+, ResNet50)

}  // namespace sqdet
