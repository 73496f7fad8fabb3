// Boxes and labels drawn into a batch of device images (sqdet_draw_items, sqdet_draw_build_items; include/sqdet.h): the
// reference's _draw_box of the training image summary (src/train.py:51-99), imdb.visualize_detections and the demos, which
// draw with cv2 / PIL on the host one image at a time.
//
// Gather, not scatter.  A rasteriser that walks the items and writes their pixels needs an order between items that overlap
// (the painter's order is part of the contract) -- atomics or one launch per item.  Here every OUTPUT pixel walks the items
// of its image in order and keeps the last one that covers it: one launch, no pixel has two writers, the result cannot depend
// on scheduling, and the image is read once and written once whatever the number of items.
//
// Work split.  The batch is one flat run of n*h*w pixels cut into chunks of CHUNK pixels, one workgroup each; a lane owns 4
// consecutive pixels at a time: 48 bytes of float32 input (three 16-byte loads), 24 of float16 (three 8-byte loads) or 12 of
// uint8, and ONE 12-byte store.  Flat, so that a group of 4 is aligned whatever the width is (a row of 1242 pixels is not a
// multiple of 16 bytes).  A chunk is a band of ~3 rows of a 1248-wide image; per image it touches (nearly always one) the
// workgroup stages that image's items -- one item per thread, <= 256 -- and keeps in LDS, in order, only those whose rectangle
// or label meets the band's rows.  A group that straddles two images, or the tail of the batch, goes element by element.
//
// -ffp-contract=off (build.py): the restore rule rint(float32(x) + mean) and bbox_transform's cx - w/2 are single roundings.
#include "draw_items.h"

namespace sqdet {
namespace {

#define SQDET_FONT5X7_DECL static const unsigned char kFontHost
#include "font5x7.h"
#undef SQDET_FONT5X7_DECL
#define SQDET_FONT5X7_DECL __constant__ unsigned char kFontDev
#include "font5x7.h"
#undef SQDET_FONT5X7_DECL

constexpr int THREADS = ITEM_THREADS;              // one item per thread at staging
constexpr int PX = 4;                              // pixels per lane and step
constexpr int STEPS = 4;
constexpr int CHUNK = THREADS * PX * STEPS;        // 4096 pixels per workgroup
constexpr int GLYPHS = 95;

struct Staged {               // an item as the pixels test it
  int xa, ya, xb, yb;         // the rectangle, corners ordered
  int lx, ly;                 // the first text cell's top-left pixel
  int len;
  uint32_t colour;            // b | g << 8 | r << 16
  unsigned char label[32];
};

struct DrawArgs {
  const void* in;
  unsigned char* out;
  int in_type, n, h, w, rgb_out, n_tables;
  float mean[3];
  const unsigned char* items[SQDET_DRAW_MAX_TABLES];
  const int32_t* counts[SQDET_DRAW_MAX_TABLES];
  int cap[SQDET_DRAW_MAX_TABLES];
};

struct alignas(4) Bytes12 { uint32_t v[3]; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// rint(float32(x) + mean) clamped to [0, 255]; NaN -> 0
__device__ __forceinline__ uint32_t restore(float x, float mean) {
  const float f = __builtin_rintf(x + mean);
  return (uint32_t)(f >= 255.0f ? 255.0f : (f > 0.0f ? f : 0.0f));
}
__device__ __forceinline__ uint32_t pack_bgr(uint32_t b, uint32_t g, uint32_t r) { return b | (g << 8) | (r << 16); }

__device__ __forceinline__ uint32_t load_pixel(const DrawArgs& a, int64_t p) {
  if (a.in_type == SQDET_F32) {
    const float* s = reinterpret_cast<const float*>(a.in) + p * 3;
    return pack_bgr(restore(s[0], a.mean[0]), restore(s[1], a.mean[1]), restore(s[2], a.mean[2]));
  }
  if (a.in_type == SQDET_F16) {
    const f16* s = reinterpret_cast<const f16*>(a.in) + p * 3;
    return pack_bgr(restore((float)s[0], a.mean[0]), restore((float)s[1], a.mean[1]), restore((float)s[2], a.mean[2]));
  }
  const unsigned char* s = reinterpret_cast<const unsigned char*>(a.in) + p * 3;
  return pack_bgr(s[0], s[1], s[2]);
}

// The 4 pixels of the aligned group starting at pixel p (p % 4 == 0, all four inside the batch).
__device__ __forceinline__ void load_group(const DrawArgs& a, int64_t p, uint32_t px[PX]) {
  if (a.in_type == SQDET_F32) {
    const f32x4* s = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(a.in) + p * 3);
    const f32x4 v0 = s[0], v1 = s[1], v2 = s[2];
    const float v[12] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3], v2[0], v2[1], v2[2], v2[3]};
#pragma unroll
    for (int k = 0; k < PX; ++k)
      px[k] = pack_bgr(restore(v[3 * k], a.mean[0]), restore(v[3 * k + 1], a.mean[1]), restore(v[3 * k + 2], a.mean[2]));
  } else if (a.in_type == SQDET_F16) {
    const f16x4* s = reinterpret_cast<const f16x4*>(reinterpret_cast<const f16*>(a.in) + p * 3);
    const f16x4 v0 = s[0], v1 = s[1], v2 = s[2];
    const float v[12] = {(float)v0[0], (float)v0[1], (float)v0[2], (float)v0[3], (float)v1[0], (float)v1[1],
                         (float)v1[2], (float)v1[3], (float)v2[0], (float)v2[1], (float)v2[2], (float)v2[3]};
#pragma unroll
    for (int k = 0; k < PX; ++k)
      px[k] = pack_bgr(restore(v[3 * k], a.mean[0]), restore(v[3 * k + 1], a.mean[1]), restore(v[3 * k + 2], a.mean[2]));
  } else {
    const Bytes12 v = *reinterpret_cast<const Bytes12*>(reinterpret_cast<const unsigned char*>(a.in) + p * 3);
    px[0] = v.v[0] & 0xffffffu;
    px[1] = (v.v[0] >> 24) | ((v.v[1] & 0xffffu) << 8);
    px[2] = (v.v[1] >> 16) | ((v.v[2] & 0xffu) << 16);
    px[3] = v.v[2] >> 8;
  }
}

// b | g << 8 | r << 16 in the output's channel order
__device__ __forceinline__ uint32_t out_order(uint32_t c, int rgb_out) {
  return rgb_out ? (((c >> 16) & 0xffu) | (c & 0xff00u) | ((c & 0xffu) << 16)) : c;
}

__device__ __forceinline__ void store_group(const DrawArgs& a, int64_t p, const uint32_t px[PX]) {
  uint32_t c[PX];
#pragma unroll
  for (int k = 0; k < PX; ++k) c[k] = out_order(px[k], a.rgb_out);
  Bytes12 v;
  v.v[0] = c[0] | (c[1] << 24);
  v.v[1] = (c[1] >> 8) | (c[2] << 16);
  v.v[2] = (c[2] >> 16) | (c[3] << 8);
  *reinterpret_cast<Bytes12*>(a.out + p * 3) = v;
}

__device__ __forceinline__ void store_pixel(const DrawArgs& a, int64_t p, uint32_t px) {
  const uint32_t c = out_order(px, a.rgb_out);
  unsigned char* d = a.out + p * 3;
  d[0] = (unsigned char)(c & 0xffu);
  d[1] = (unsigned char)((c >> 8) & 0xffu);
  d[2] = (unsigned char)((c >> 16) & 0xffu);
}

// What item e makes of pixel (x, y): its colour where its rectangle's outline or a set bit of its label lies, else `px`.
__device__ __forceinline__ uint32_t paint(const Staged& e, const unsigned char* font, int x, int y, uint32_t px) {
  if (x >= e.xa && x <= e.xb && y >= e.ya && y <= e.yb && (x == e.xa || x == e.xb || y == e.ya || y == e.yb)) px = e.colour;
  // (unsigned differences: a pixel left of / above the text wraps to a huge value and fails both tests)
  const unsigned dx = (unsigned)x - (unsigned)e.lx, dy = (unsigned)y - (unsigned)e.ly;
  if (dy < 7u && dx < 6u * (unsigned)e.len) {
    const unsigned ci = dx / 6u, cx = dx - 6u * ci;
    if (cx != 0u) {
      const unsigned ch = e.label[ci];
      const unsigned gi = (ch >= 32u && ch <= 126u) ? ch - 32u : (unsigned)('?' - 32);
      if ((font[gi * 8u + dy] >> (5u - cx)) & 1u) px = e.colour;
    }
  }
  return px;
}

__global__ void __launch_bounds__(THREADS) draw_kernel(const DrawArgs a) {
  __shared__ Staged s_item[SQDET_DRAW_MAX_ITEMS];
  __shared__ unsigned char s_font[GLYPHS * 8];
  __shared__ int s_wave[THREADS / 64];
  const int tid = threadIdx.x;
  for (int i = tid; i < GLYPHS * 7; i += THREADS) s_font[(i / 7) * 8 + i % 7] = kFontDev[i / 7][i % 7];

  const int64_t hw = (int64_t)a.h * a.w, total = hw * a.n;
  const int64_t c0 = (int64_t)blockIdx.x * CHUNK;
  const int64_t c1 = c0 + CHUNK < total ? c0 + CHUNK : total;
  if (c0 >= c1) return;
  const int b_first = (int)(c0 / hw), b_last = (int)((c1 - 1) / hw);
  for (int b = b_first; b <= b_last; ++b) {
    const int64_t img0 = (int64_t)b * hw;
    const int64_t s0 = c0 > img0 ? c0 : img0, s1 = c1 < img0 + hw ? c1 : img0 + hw;      // this image's pixels of the chunk
    const int ylo = (int)((s0 - img0) / a.w), yhi = (int)((s1 - 1 - img0) / a.w);
    __syncthreads();          // the previous image's items are no longer read (first pass: the font is in place)
    // ---- stage: thread t takes the t-th item of image b over all tables, keeps it if it meets rows [ylo, yhi]
    const unsigned char* src = nullptr;
    int t = tid;
    for (int k = 0; k < a.n_tables && src == nullptr; ++k) {
      const int cnt = clampi(a.counts[k][b], 0, a.cap[k]);
      if (t < cnt) src = a.items[k] + ((size_t)b * a.cap[k] + t) * SQDET_DRAW_ITEM_BYTES;
      t -= cnt;
    }
    bool hit = false;
    Staged e;
    if (src != nullptr) {
      const i32x4* q = reinterpret_cast<const i32x4*>(src);
      const i32x4 r0 = q[0], r1 = q[1], r2 = q[2], r3 = q[3];
      const int x0 = clampi(r0[0], -COORD_LIM, COORD_LIM), y0 = clampi(r0[1], -COORD_LIM, COORD_LIM);
      const int x1 = clampi(r0[2], -COORD_LIM, COORD_LIM), y1 = clampi(r0[3], -COORD_LIM, COORD_LIM);
      const uint32_t cw = (uint32_t)r1[0];
      e.xa = x0 < x1 ? x0 : x1; e.xb = x0 < x1 ? x1 : x0;
      e.ya = y0 < y1 ? y0 : y1; e.yb = y0 < y1 ? y1 : y0;
      e.colour = cw & 0xffffffu;
      e.len = clampi(r1[1], 0, SQDET_DRAW_LABEL_MAX);
      e.lx = x0;
      e.ly = ((cw >> 24) == SQDET_DRAW_TOP_LEFT) ? y0 : y1 - 7;
      const int lab[8] = {r1[2], r1[3], r2[0], r2[1], r2[2], r2[3], r3[0], r3[1]};
#pragma unroll
      for (int i = 0; i < 8; ++i) reinterpret_cast<int*>(e.label)[i] = lab[i];
      const bool rect = e.ya <= yhi && e.yb >= ylo && e.xa <= a.w - 1 && e.xb >= 0;
      const bool text = e.len > 0 && e.ly <= yhi && e.ly + 6 >= ylo && e.lx <= a.w - 1 && e.lx + 6 * e.len - 1 >= 0;
      hit = rect || text;
    }
    int kept;
    const int pos = block_compact(hit, s_wave, &kept);
    if (hit) s_item[pos] = e;
    __syncthreads();
    // ---- paint
    for (int step = 0; step < STEPS; ++step) {
      const int64_t g0 = c0 + ((int64_t)step * THREADS + tid) * PX;
      const int64_t lo = g0 > s0 ? g0 : s0, hi = g0 + PX < s1 ? g0 + PX : s1;
      if (lo >= hi) continue;
      const bool full = hi - lo == PX;
      uint32_t px[PX] = {0, 0, 0, 0};
      if (full) {
        load_group(a, g0, px);
      } else {
#pragma unroll
        for (int k = 0; k < PX; ++k)
          if (g0 + k >= lo && g0 + k < hi) px[k] = load_pixel(a, g0 + k);
      }
      if (kept > 0) {
        const int r = (int)(lo - img0);
        int yk[PX], xk[PX];
        int y = r / a.w, x = r - y * a.w;
#pragma unroll
        for (int k = 0; k < PX; ++k) {
          const bool in = g0 + k >= lo && g0 + k < hi;
          xk[k] = in ? x : -1;       // (-1: not this pass's pixel)
          yk[k] = in ? y : -1;
          if (in && ++x == a.w) { x = 0; ++y; }
        }
        for (int i = 0; i < kept; ++i) {
          const Staged& it = s_item[i];
#pragma unroll
          for (int k = 0; k < PX; ++k)
            if (xk[k] >= 0) px[k] = paint(it, s_font, xk[k], yk[k], px[k]);
        }
      }
      if (full) {
        store_group(a, g0, px);
      } else {
#pragma unroll
        for (int k = 0; k < PX; ++k)
          if (g0 + k >= lo && g0 + k < hi) store_pixel(a, g0 + k, px[k]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ item builder
// build_items_kernel's rule (draw_items.h) for detection or ground-truth rows: float32 or float64 boxes, centre or diagonal,
// one colour or one per class, "<name>", "<name>: (p)" or "<name> (p)".
struct DetectionRule {
  const void* boxes;
  const unsigned char* class_bgr;
  int boxes_f64, diagonal, label_format;
  uint32_t fixed;             // b | g << 8 | r << 16
  __device__ bool keep(size_t) const { return true; }
  __device__ void corners(size_t row, double v[4]) const {
    if (boxes_f64) corners_of(reinterpret_cast<const double*>(boxes) + row * 4, diagonal, v);
    else corners_of(reinterpret_cast<const float*>(boxes) + row * 4, diagonal, v);
  }
  __device__ uint32_t colour(size_t, int c, bool known) const {
    if (!known || class_bgr == nullptr) return fixed;
    const unsigned char* q = class_bgr + (size_t)c * 3;
    return pack_bgr(q[0], q[1], q[2]);
  }
  __device__ void label(LabelWriter& w, const ItemArgs& a, size_t row) const {
    if (label_format == SQDET_DRAW_LABEL_NAME) return;
    w.puts(label_format == SQDET_DRAW_LABEL_NAME_COLON_PROB ? ": (" : " (");
    w.fixed2((double)a.probs[row]);       // (the entry point requires probs for these formats)
    w.put(')');
  }
};

}  // namespace
}  // namespace sqdet

using namespace sqdet;

extern "C" int sqdet_draw_font5x7(unsigned char* host_out, size_t capacity) {
  SQDET_REQUIRE(host_out != nullptr, "sqdet_draw_font5x7: null pointer");
  SQDET_REQUIRE(capacity >= sizeof(kFontHost), "sqdet_draw_font5x7: %zu bytes, the table has %zu", capacity, sizeof(kFontHost));
  for (int g = 0; g < GLYPHS; ++g)
    for (int r = 0; r < 7; ++r) host_out[g * 7 + r] = kFontHost[g][r];
  return SQDET_OK;
}

extern "C" int sqdet_draw_items(const void* images, unsigned char* out, int in_type, int n, int h, int w,
                                const float* host_bgr_means, int rgb_out, const void* const* item_tables,
                                const int32_t* const* item_counts, const int* caps, int n_tables, sqdet_stream_t stream) {
  SQDET_REQUIRE(images != nullptr && out != nullptr, "sqdet_draw_items: null pointer");
  SQDET_REQUIRE(in_type == SQDET_F32 || in_type == SQDET_F16 || in_type == SQDET_DRAW_U8, "sqdet_draw_items: bad in_type %d", in_type);
  SQDET_REQUIRE(in_type == SQDET_DRAW_U8 || host_bgr_means != nullptr, "sqdet_draw_items: null means for a float input");
  SQDET_REQUIRE(n > 0 && h > 0 && w > 0, "sqdet_draw_items: bad shape %d x %d x %d", n, h, w);
  SQDET_REQUIRE(n_tables >= 0 && n_tables <= SQDET_DRAW_MAX_TABLES, "sqdet_draw_items: %d tables (0 .. %d)", n_tables, SQDET_DRAW_MAX_TABLES);
  SQDET_REQUIRE(n_tables == 0 || (item_tables != nullptr && item_counts != nullptr && caps != nullptr), "sqdet_draw_items: null table list");
  DrawArgs a{};
  long long items = 0;
  for (int k = 0; k < n_tables; ++k) {
    SQDET_REQUIRE(item_tables[k] != nullptr && item_counts[k] != nullptr, "sqdet_draw_items: null pointer in table %d", k);
    SQDET_REQUIRE(caps[k] > 0, "sqdet_draw_items: capacity %d of table %d", caps[k], k);
    SQDET_REQUIRE((reinterpret_cast<uintptr_t>(item_tables[k]) & 15) == 0, "sqdet_draw_items: table %d is not 16-byte aligned", k);
    a.items[k] = reinterpret_cast<const unsigned char*>(item_tables[k]);
    a.counts[k] = item_counts[k];
    a.cap[k] = caps[k];
    items += caps[k];
  }
  SQDET_UNSUPPORTED(items > SQDET_DRAW_MAX_ITEMS, "sqdet_draw_items: %lld items per image (at most %d)", items, SQDET_DRAW_MAX_ITEMS);
  SQDET_UNSUPPORTED((long long)h * w > 0x7fffffffLL / n, "sqdet_draw_items: %d x %d x %d pixels (at most 2^31 - 1)", n, h, w);
  const long long total = (long long)n * h * w;
  // (a lane reads and writes groups of 4 pixels with vector accesses: 48 / 24 / 12 bytes in, 12 bytes out)
  const uintptr_t in_align = in_type == SQDET_F32 ? 15 : (in_type == SQDET_F16 ? 7 : 3);
  SQDET_REQUIRE((reinterpret_cast<uintptr_t>(images) & in_align) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                "sqdet_draw_items: images must be %d-byte aligned, out 4-byte", (int)in_align + 1);
  a.in = images; a.out = out; a.in_type = in_type; a.n = n; a.h = h; a.w = w; a.rgb_out = rgb_out ? 1 : 0; a.n_tables = n_tables;
  for (int c = 0; c < 3; ++c) a.mean[c] = in_type == SQDET_DRAW_U8 ? 0.0f : host_bgr_means[c];
  const unsigned grid = (unsigned)((total + CHUNK - 1) / CHUNK);
  hipLaunchKernelGGL(draw_kernel, dim3(grid), dim3(THREADS), 0, as_stream(stream), a);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" int sqdet_draw_build_items(const void* boxes, int boxes_f64, const float* probs, const int32_t* cls,
                                      const int32_t* counts, int n, int rows, int diagonal, double plot_thresh,
                                      const unsigned char* names, int classes, const unsigned char* class_bgr, int b, int g,
                                      int r, int label_format, int anchor, void* items, int32_t* item_counts, int cap,
                                      sqdet_stream_t stream) {
  SQDET_REQUIRE(boxes != nullptr && cls != nullptr && counts != nullptr && names != nullptr && items != nullptr && item_counts != nullptr,
                "sqdet_draw_build_items: null pointer");
  SQDET_REQUIRE(n > 0 && rows > 0 && classes > 0 && cap > 0, "sqdet_draw_build_items: bad sizes n %d rows %d classes %d cap %d", n, rows, classes, cap);
  SQDET_REQUIRE(label_format >= SQDET_DRAW_LABEL_NAME && label_format <= SQDET_DRAW_LABEL_NAME_PROB, "sqdet_draw_build_items: bad label_format %d", label_format);
  SQDET_REQUIRE(label_format == SQDET_DRAW_LABEL_NAME || probs != nullptr, "sqdet_draw_build_items: a label with a probability needs probs");
  SQDET_REQUIRE(((b | g | r) & ~0xff) == 0, "sqdet_draw_build_items: colour (%d, %d, %d)", b, g, r);
  ItemArgs a{};
  a.probs = probs; a.cls = cls; a.counts = counts; a.names = names; a.items = reinterpret_cast<unsigned char*>(items);
  a.item_counts = item_counts; a.rows = rows; a.classes = classes; a.anchor = anchor; a.cap = cap; a.plot_thresh = plot_thresh;
  const DetectionRule rule{boxes, class_bgr, boxes_f64 ? 1 : 0, diagonal ? 1 : 0, label_format,
                           (uint32_t)b | ((uint32_t)g << 8) | ((uint32_t)r << 16)};
  return build_items("sqdet_draw_build_items", a, rule, n, stream);
}
