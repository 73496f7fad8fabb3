// Training-time image preparation of the reference's batch reader (src/dataset/imdb.py:141-186) on the GPU: per image
//   im = imread(f).astype(float32);  im -= mc.BGR_MEANS            (float64 means: (float)((double)v - mean), rounded once)
//   drift by (dx, dy): D[i, j] = im[i + dy, j + dx] inside im, 0.0 outside, D is (H - dy) x (W - dx)
//   flip: D[i, j] = D[i, W' - 1 - j]
//   out = cv2.resize(D, (dst_w, dst_h))                              (INTER_LINEAR, float32, coordinates as preproc.hip)
// -> one launch for a batch of images of different sizes, each at its own byte offset of one flat uint8 buffer.
//
// sqdet_augment_bgr_window generalises the drift to a WINDOW (x0, y0, cw, ch) in original-image coordinates -- inside the image
// (a crop), around it (zoom-out: the padding is 0.0f, the mean colour) or across an edge -- and can apply a 3x4 colour matrix
// to the bytes of every source pixel, clamped to [0, 255], before the mean is subtracted.  The drift is the window
// (dx, dy, w - dx, h - dy) without a matrix; both entry points instantiate the one kernel body below.
//
// Unlike sqdet_preprocess_bgr (demo.py's order: resize, then subtract the mean) the mean is subtracted BEFORE the
// interpolation, so the kernel interpolates the float32 mean-subtracted values and the zero padding stays exactly 0.0f.
// Built with -ffp-contract=off: the same float32 operations in the same order as the CPU restatement.
//
// sqdet_augment_bgr_mosaic cuts every output image at (xc, yc) into four panes and fills each pane with the window form of its own
// source image, resized to the pane: the same body once more, with the pane in place of the destination image.
#include "common.h"

namespace sqdet {

// Same layout as preprocess_kernel: one 64-thread workgroup = 256 consecutive pixels of one destination row (4 per thread);
// the image's geometry, its two source rows and the vertical weight are workgroup-uniform; a source pixel pair is one
// unaligned 8-byte load (reversed when mirrored) wherever both pixels lie inside the image.
constexpr int APX = 4;   // destination pixels per thread

// dx, dy: the window's corner in the original image; the window D is Hs x Ws
struct AugGeom {
  int h, w, dx, dy, flip;
};

// float32 value of channel c of the pixel whose 3 bytes start at bit 24*k of q, mean-subtracted in double
__device__ __forceinline__ float sub_mean(unsigned long long q, int k, int c, double mean) {
  return (float)((double)(unsigned)((q >> (24 * k + 8 * c)) & 255) - mean);
}

// the same after the colour matrix M (row c of a row-major 3x4: three gains on b, g, r and an offset), clamped to [0, 255]
__device__ __forceinline__ float color_sub_mean(unsigned long long q, int k, int c, const float* M, double mean) {
  const float b = (float)(unsigned)((q >> (24 * k)) & 255), g = (float)(unsigned)((q >> (24 * k + 8)) & 255);
  const float r = (float)(unsigned)((q >> (24 * k + 16)) & 255);
  float v = ((M[4 * c] * b + M[4 * c + 1] * g) + M[4 * c + 2] * r) + M[4 * c + 3];
  v = fminf(fmaxf(v, 0.f), 255.f);
  return (float)((double)v - mean);
}

// WINDOW: geom is [n,7] (src_h, src_w, x0, y0, cw, ch, flip), else [n,5] (src_h, src_w, dx, dy, flip); COLOR: color is [n,12].
// MOSAIC (with WINDOW): offsets, geom and color hold FOUR rows per image, one per pane, and split [n,2] = (xc, yc) cuts the image;
// the grid has one more workgroup per row, each side of xc is covered by its own 256-pixel chunks (the left side's first), so the
// pane -- and with it the geometry -- stays workgroup-uniform; Hp x Wp at (py0, px0) is the pane, the whole image without MOSAIC.
template <typename T, bool WINDOW, bool COLOR, bool MOSAIC = false>
__global__ __launch_bounds__(64) void augment_kernel(const unsigned char* __restrict__ src, size_t src_bytes,
                                                     const int64_t* __restrict__ offsets, const int32_t* __restrict__ geom,
                                                     const float* __restrict__ color, T* __restrict__ dst, int Hd, int Wd,
                                                     double m0, double m1, double m2, const int32_t* __restrict__ split) {
  static_assert(WINDOW || !MOSAIC, "a mosaic pane is a window");
  const int row = blockIdx.y;                     // n * Hd + y
  int n = row / Hd, y = row - n * Hd;
  constexpr int GS = WINDOW ? 7 : 5;
  int Hp = Hd, Wp = Wd, px0 = 0, chunk = blockIdx.x;
  if constexpr (MOSAIC) {
    const int xc = split[2 * n], yc = split[2 * n + 1];
    if (xc < 0 || xc > Wd || yc < 0 || yc > Hd) return;          // (rejected by the host wrapper) the image is left unwritten
    const int nl = (xc + 64 * APX - 1) / (64 * APX);             // chunks of the left side; an empty pane gets no workgroup
    const bool right = chunk >= nl, bottom = y >= yc;
    if (right) { chunk -= nl; px0 = xc; Wp = Wd - xc; } else Wp = xc;
    if (bottom) { y -= yc; Hp = Hd - yc; } else Hp = yc;
    if (chunk * 64 * APX >= Wp) return;
    n = 4 * n + 2 * (int)bottom + (int)right;                    // the pane's row of offsets, geom and color
  }
  const AugGeom g{geom[GS * n], geom[GS * n + 1], geom[GS * n + 2], geom[GS * n + 3], geom[GS * n + GS - 1]};
  const int64_t off = offsets[n];
  int Hs, Ws;                                      // the window D: the drifted image, or (ch, cw)
  // the host wrapper rejects all of these before the launch; an image that gets here anyway is left unwritten
  if (g.h <= 0 || g.w <= 0 || g.dx < -65535 || g.dx > 65535 || g.dy < -65535 || g.dy > 65535 || (g.flip & ~1) || off < 0 ||
      (size_t)off > src_bytes || (size_t)g.h * g.w * 3 > src_bytes - (size_t)off)
    return;
  if constexpr (WINDOW) {
    Ws = geom[GS * n + 4];
    Hs = geom[GS * n + 5];
    // (above 65535 only the drift's own window, which ends at the image's far edge: what sqdet_augment_bgr accepts)
    if (Ws < 1 || (Ws > 65535 && (long)g.dx + Ws != g.w) || Hs < 1 || (Hs > 65535 && (long)g.dy + Hs != g.h)) return;
  } else {
    if (g.dx >= g.w || g.dy >= g.h) return;
    Hs = g.h - g.dy;
    Ws = g.w - g.dx;
  }
  float M[COLOR ? 12 : 1];
  if constexpr (COLOR) {
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = color[12 * n + k];
  }
  const double scale_x = (double)Ws / (double)Wp, scale_y = (double)Hs / (double)Hp;
  float fy = (float)((y + 0.5) * scale_y - 0.5);
  int sy = (int)floorf(fy);
  fy -= sy;
  if (sy < 0) { sy = 0; fy = 0.f; }
  if (sy >= Hs - 1) { sy = Hs - 1; fy = 0.f; }
  const int sy1 = sy + 1 < Hs ? sy + 1 : sy;
  const int oy0 = sy + g.dy, oy1 = sy1 + g.dy;    // rows of the original image (outside [0, h): zero padding)
  const bool r0 = oy0 >= 0 && oy0 < g.h, r1 = oy1 >= 0 && oy1 < g.h;
  const size_t o0 = (size_t)off + (size_t)(r0 ? oy0 : 0) * g.w * 3, o1 = (size_t)off + (size_t)(r1 ? oy1 : 0) * g.w * 3;
  const float ay0 = 1.f - fy;
  const double mean[3] = {m0, m1, m2};
  const int x0 = (chunk * 64 + threadIdx.x) * APX;     // in the pane
  if (x0 >= Wp) return;
  float out[APX * 3];
#pragma unroll
  for (int p = 0; p < APX; ++p) {
    const int x = x0 + p < Wp ? x0 + p : Wp - 1;
    float fx = (float)((x + 0.5) * scale_x - 0.5);
    int sx = (int)floorf(fx);
    fx -= sx;
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= Ws - 1) { sx = Ws - 1; fx = 0.f; }
    const int sx1 = sx + 1 < Ws ? sx + 1 : sx;
    const float ax0 = 1.f - fx;
    // original columns of D's columns sx and sx1 (mirrored: W' - 1 - column)
    const int ox = (g.flip ? Ws - 1 - sx : sx) + g.dx, ox1 = (g.flip ? Ws - 1 - sx1 : sx1) + g.dx;
    const bool c0 = ox >= 0 && ox < g.w, c1 = ox1 >= 0 && ox1 < g.w;
    // q*: pixel sx in bytes [0, 3), pixel sx1 in bytes [3, 6); ok*: which of the four values are inside the image
    unsigned long long q0 = 0, q1 = 0;
    bool ok00 = r0 && c0, ok01 = r0 && c1, ok10 = r1 && c0, ok11 = r1 && c1;
    const int lo = ox < ox1 ? ox : ox1;           // the pair's left original column (ox1 = ox -+ 1 off the last column)
    const size_t b0 = o0 + (size_t)lo * 3, b1 = o1 + (size_t)lo * 3;
    if (sx1 != sx && ok00 && ok01 && ok10 && ok11 && b0 + 8 <= src_bytes && b1 + 8 <= src_bytes) {
      q0 = *reinterpret_cast<const unsigned long long*>(src + b0);
      q1 = *reinterpret_cast<const unsigned long long*>(src + b1);
      if (g.flip) {                                // the pair arrives as (ox - 1, ox): swap the two pixels
        q0 = ((q0 >> 24) & 0xffffffull) | ((q0 & 0xffffffull) << 24);
        q1 = ((q1 >> 24) & 0xffffffull) | ((q1 & 0xffffffull) << 24);
      }
    } else {                                       // padding, the last column, or the end of the buffer: byte loads
      const size_t a00 = o0 + (size_t)(c0 ? ox : 0) * 3, a01 = o0 + (size_t)(c1 ? ox1 : 0) * 3;
      const size_t a10 = o1 + (size_t)(c0 ? ox : 0) * 3, a11 = o1 + (size_t)(c1 ? ox1 : 0) * 3;
      ok00 = ok00 && a00 + 3 <= src_bytes;
      ok01 = ok01 && a01 + 3 <= src_bytes;
      ok10 = ok10 && a10 + 3 <= src_bytes;
      ok11 = ok11 && a11 + 3 <= src_bytes;
      for (int k = 0; k < 3; ++k) {
        if (ok00) q0 |= (unsigned long long)src[a00 + k] << (8 * k);
        if (ok01) q0 |= (unsigned long long)src[a01 + k] << (8 * (k + 3));
        if (ok10) q1 |= (unsigned long long)src[a10 + k] << (8 * k);
        if (ok11) q1 |= (unsigned long long)src[a11 + k] << (8 * (k + 3));
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float s00, s01, s10, s11;                      // padding stays 0.0f: neither the matrix nor the mean touches it
      if constexpr (COLOR) {
        s00 = ok00 ? color_sub_mean(q0, 0, c, M, mean[c]) : 0.f, s01 = ok01 ? color_sub_mean(q0, 1, c, M, mean[c]) : 0.f;
        s10 = ok10 ? color_sub_mean(q1, 0, c, M, mean[c]) : 0.f, s11 = ok11 ? color_sub_mean(q1, 1, c, M, mean[c]) : 0.f;
      } else {
        s00 = ok00 ? sub_mean(q0, 0, c, mean[c]) : 0.f, s01 = ok01 ? sub_mean(q0, 1, c, mean[c]) : 0.f;
        s10 = ok10 ? sub_mean(q1, 0, c, mean[c]) : 0.f, s11 = ok11 ? sub_mean(q1, 1, c, mean[c]) : 0.f;
      }
      const float h0 = s00 * ax0 + s01 * fx;
      const float h1 = s10 * ax0 + s11 * fx;
      out[p * 3 + c] = h0 * ay0 + h1 * fy;
    }
  }
  T* d = dst + ((size_t)row * Wd + px0 + x0) * 3;
  if (x0 + APX <= Wp && (reinterpret_cast<uintptr_t>(d) & 7) == 0) {
    if constexpr (sizeof(T) == 2) {
      typedef f16 h4 __attribute__((ext_vector_type(4)));
#pragma unroll
      for (int k = 0; k < 3; ++k)
        reinterpret_cast<h4*>(d)[k] = h4{(f16)out[4 * k], (f16)out[4 * k + 1], (f16)out[4 * k + 2], (f16)out[4 * k + 3]};
    } else {
      typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
      for (int k = 0; k < 6; ++k) reinterpret_cast<f2*>(d)[k] = f2{out[2 * k], out[2 * k + 1]};
    }
  } else if (sizeof(T) == 2 && x0 + APX <= Wp && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
    typedef f16 h2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int k = 0; k < 6; ++k) reinterpret_cast<h2*>(d)[k] = h2{(f16)out[2 * k], (f16)out[2 * k + 1]};
  } else {
    for (int p = 0; p < APX && x0 + p < Wp; ++p)
      for (int c = 0; c < 3; ++c) d[p * 3 + c] = (T)out[p * 3 + c];
  }
}

template <bool WINDOW, bool COLOR, bool MOSAIC = false>
static int launch_augment(const char* name, const uint8_t* src, size_t src_bytes, const int64_t* src_offsets, const int32_t* geom,
                          const int32_t* split, const float* color, void* dst, int n, int dst_h, int dst_w, double mean_b, double mean_g, double mean_r,
                          int dtype, sqdet_stream_t stream) {
  SQDET_REQUIRE(src && src_offsets && geom && dst && (split || !MOSAIC), "%s: null pointer", name);
  SQDET_REQUIRE(n > 0 && dst_h > 0 && dst_w > 0 && src_bytes > 0, "%s: bad dims", name);
  SQDET_REQUIRE(dtype == SQDET_F16 || dtype == SQDET_F32, "%s: bad dtype %d", name, dtype);
  SQDET_REQUIRE((long)n * dst_h <= 0x7fffffffL / 4, "%s: too many rows", name);
  const dim3 grid((unsigned)((dst_w + 64 * APX - 1) / (64 * APX)) + (MOSAIC ? 1u : 0u), (unsigned)(n * dst_h));
  SQDET_REQUIRE(grid.y <= 65535u * 1024u, "%s: too many rows", name);
  if (dtype == SQDET_F16)
    hipLaunchKernelGGL((augment_kernel<f16, WINDOW, COLOR, MOSAIC>), grid, dim3(64), 0, as_stream(stream), src, src_bytes, src_offsets,
                       geom, color, (f16*)dst, dst_h, dst_w, mean_b, mean_g, mean_r, split);
  else
    hipLaunchKernelGGL((augment_kernel<float, WINDOW, COLOR, MOSAIC>), grid, dim3(64), 0, as_stream(stream), src, src_bytes, src_offsets,
                       geom, color, (float*)dst, dst_h, dst_w, mean_b, mean_g, mean_r, split);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

}  // namespace sqdet

extern "C" int sqdet_augment_bgr(const uint8_t* src, size_t src_bytes, const int64_t* src_offsets, const int32_t* geom,
                                 void* dst, int n, int dst_h, int dst_w, double mean_b, double mean_g, double mean_r,
                                 int dtype, sqdet_stream_t stream) {
  return sqdet::launch_augment<false, false>("augment_bgr", src, src_bytes, src_offsets, geom, nullptr, nullptr, dst, n, dst_h, dst_w, mean_b,
                                             mean_g, mean_r, dtype, stream);
}

extern "C" int sqdet_augment_bgr_window(const uint8_t* src, size_t src_bytes, const int64_t* src_offsets, const int32_t* geom,
                                        const float* color, void* dst, int n, int dst_h, int dst_w, double mean_b, double mean_g,
                                        double mean_r, int dtype, sqdet_stream_t stream) {
  const auto launch = color ? sqdet::launch_augment<true, true> : sqdet::launch_augment<true, false>;
  return launch("augment_bgr_window", src, src_bytes, src_offsets, geom, nullptr, color, dst, n, dst_h, dst_w, mean_b, mean_g, mean_r, dtype,
                stream);
}

extern "C" int sqdet_augment_bgr_mosaic(const uint8_t* src, size_t src_bytes, const int64_t* part_offsets, const int32_t* geom,
                                        const int32_t* split, const float* color, void* dst, int n, int dst_h, int dst_w, double mean_b,
                                        double mean_g, double mean_r, int dtype, sqdet_stream_t stream) {
  const auto launch = color ? sqdet::launch_augment<true, true, true> : sqdet::launch_augment<true, false, true>;
  return launch("augment_bgr_mosaic", src, src_bytes, part_offsets, geom, split, color, dst, n, dst_h, dst_w, mean_b, mean_g, mean_r,
                dtype, stream);
}
