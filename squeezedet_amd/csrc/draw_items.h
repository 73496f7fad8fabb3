// The 64-byte drawing item (include/sqdet.h, "drawing") and the one kernel that builds item tables from box rows:
// sqdet_draw_build_items (draw.hip) and sqdet_track_build_items (track.hip) instantiate build_items_kernel<Rule> with what they
// keep, how they colour and label a row, and the form of their boxes.  draw.hip's rasteriser reads the same struct.
// Build with -ffp-contract=off: bbox_transform's cx - w/2 is a single rounding, the label's '%.2f' is round_decimal.h's.
#pragma once
#include <stddef.h>
#include "common.h"
#include "round_decimal.h"
#include "stream_wave.h"

namespace sqdet {
namespace {

constexpr int ITEM_THREADS = SQDET_DRAW_MAX_ITEMS;  // one row, or one item, per thread of a workgroup
constexpr int COORD_LIM = 1 << 30;

struct Item {                 // include/sqdet.h, "drawing"
  int32_t x0, y0, x1, y1;
  uint8_t b, g, r, anchor;
  int32_t label_len;
  unsigned char label[32];
  int32_t pad[2];
};
static_assert(sizeof(Item) == SQDET_DRAW_ITEM_BYTES && SQDET_DRAW_ITEM_BYTES == 64, "item layout");
static_assert(offsetof(Item, x0) == 0 && offsetof(Item, y1) == 12 && offsetof(Item, b) == 16 && offsetof(Item, anchor) == 19 &&
                  offsetof(Item, label_len) == 20 && offsetof(Item, label) == 24 && offsetof(Item, pad) == 56,
              "item layout");

// int(): truncation toward zero, clamped to the range the rasteriser uses; NaN -> 0
__device__ __forceinline__ int32_t to_int(double v) {
  if (v != v) return 0;
  if (v >= (double)COORD_LIM) return COORD_LIM;
  if (v <= -(double)COORD_LIM) return -COORD_LIM;
  return (int32_t)v;
}

// xmin, ymin, xmax, ymax of a row: the row itself (diagonal), or util.bbox_transform of (cx, cy, w, h) in the row's own precision --
// float32 arithmetic for a float32 row -- then widened exactly
template <class T>
__device__ __forceinline__ void corners_of(const T* s, bool diagonal, double v[4]) {
  const T xmin = s[0] - s[2] / 2, ymin = s[1] - s[3] / 2, xmax = s[0] + s[2] / 2, ymax = s[1] + s[3] / 2;
  v[0] = diagonal ? s[0] : xmin; v[1] = diagonal ? s[1] : ymin; v[2] = diagonal ? s[2] : xmax; v[3] = diagonal ? s[3] : ymax;
}

struct LabelWriter {
  unsigned char* s;
  int n;
  __device__ void put(unsigned char c) {
    if (n < SQDET_DRAW_LABEL_MAX) s[n++] = c;
  }
  __device__ void puts(const char* t) {
    for (; *t; ++t) put((unsigned char)*t);
  }
  // '%d' % v, v >= 0
  __device__ void decimal(int v) {
    char d[12];
    int nd = 0;
    do { d[nd++] = (char)('0' + v % 10); v /= 10; } while (v > 0 && nd < 12);
    while (nd > 0) put((unsigned char)d[--nd]);
  }
  // '%.2f' % v with Python's digits
  __device__ void fixed2(double v) {
    if (v != v) { puts("nan"); return; }
    if (__builtin_signbit(v)) put('-');
    const double m = __builtin_fabs(v);
    if (m == __builtin_inf()) { puts("inf"); return; }
    if (m >= 1e7) { puts("?.??"); return; }
    const long long units = (long long)round_decimal_units(m, 100.0);
    const int fp = (int)(units % 100);
    decimal((int)(units / 100));         // (< 1e7)
    put('.');
    put((unsigned char)('0' + fp / 10));
    put((unsigned char)('0' + fp % 10));
  }
};

// Ballot compaction over the ITEM_THREADS threads of a workgroup, order kept: the number of keeping threads before this one;
// *kept: of all.  s_wave: one LDS word per wave, free to be rewritten after the caller's next barrier.  Synchronises once.
__device__ __forceinline__ int block_compact(bool keep, int* s_wave, int* kept) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t mask = __ballot(keep);
  if (lane == 0) s_wave[wave] = __popcll(mask);
  __syncthreads();
  int base = 0;
  *kept = 0;
#pragma unroll
  for (int v = 0; v < ITEM_THREADS / 64; ++v) {
    if (v < wave) base += s_wave[v];
    *kept += s_wave[v];
  }
  return base + rank_in(mask, lane);
}

// What every item builder is given; a Rule holds the rest.
struct ItemArgs {
  const float* probs;         // may be NULL where the rule does not need them: then no row is cut by plot_thresh
  const int32_t* cls;
  const int32_t* counts;
  const unsigned char* names;
  unsigned char* items;
  int32_t* item_counts;
  int rows, classes, anchor, cap;
  double plot_thresh;
};

// One workgroup per image, one thread per row: image i keeps, in order, its rows j < counts[i] that the rule keeps and whose
// prob is above plot_thresh (float32 against a Python float: the reference compares in double).  Rule:
//   bool keep(row)                       the rule's own cut
//   void corners(row, v)                 xmin, ymin, xmax, ymax
//   uint32_t colour(row, c, known)       b | g << 8 | r << 16; c the row's class, known: it has a name
//   void label(w, a, row)                what follows the class name
template <class Rule>
__global__ void __launch_bounds__(ITEM_THREADS) build_items_kernel(const ItemArgs a, const Rule rule) {
  __shared__ int s_wave[ITEM_THREADS / 64];
  const int img = blockIdx.x, j = threadIdx.x;
  const int cnt = clamp_count(a.counts[img], a.rows);
  const size_t row = (size_t)img * a.rows + j;
  const bool keep = j < cnt && rule.keep(row) && (a.probs == nullptr || (double)a.probs[row] > a.plot_thresh);
  int kept;
  const int pos = block_compact(keep, s_wave, &kept);           // < cnt <= rows <= cap
  if (j == 0) a.item_counts[img] = kept;
  if (!keep) return;
  Item it;
  double v[4];
  rule.corners(row, v);
  it.x0 = to_int(v[0]); it.y0 = to_int(v[1]); it.x1 = to_int(v[2]); it.y1 = to_int(v[3]);
  const int c = a.cls[row];
  const bool known = c >= 0 && c < a.classes;
  const uint32_t colour = rule.colour(row, c, known);
  it.b = (uint8_t)(colour & 0xffu); it.g = (uint8_t)((colour >> 8) & 0xffu); it.r = (uint8_t)((colour >> 16) & 0xffu);
  it.anchor = (uint8_t)a.anchor;
  for (int i = 0; i < 32; ++i) it.label[i] = 0;
  it.pad[0] = it.pad[1] = 0;
  LabelWriter w{it.label, 0};
  if (known) {
    const unsigned char* nm = a.names + (size_t)c * SQDET_DRAW_NAME_BYTES;
    for (int i = 0; i < SQDET_DRAW_NAME_BYTES && nm[i]; ++i) w.put(nm[i]);
  } else {
    w.put('?');
  }
  rule.label(w, a, row);
  it.label_len = w.n;
  *reinterpret_cast<Item*>(a.items + ((size_t)img * a.cap + pos) * SQDET_DRAW_ITEM_BYTES) = it;
}

// The tail of sqdet_<who>, an item builder's entry point: the checks of the table it writes, then the launch over n images.
template <class Rule>
int build_items(const char* who, const ItemArgs& a, const Rule& rule, int n, sqdet_stream_t stream) {
  SQDET_REQUIRE(a.anchor == SQDET_DRAW_BOTTOM_LEFT || a.anchor == SQDET_DRAW_TOP_LEFT, "%s: bad anchor %d", who, a.anchor);
  SQDET_UNSUPPORTED(a.cap > SQDET_DRAW_MAX_ITEMS || a.rows > a.cap, "%s: %d rows into %d items per image (at most %d)", who, a.rows, a.cap,
                    SQDET_DRAW_MAX_ITEMS);
  SQDET_REQUIRE((reinterpret_cast<uintptr_t>(a.items) & 15) == 0, "%s: items must be 16-byte aligned", who);
  hipLaunchKernelGGL(build_items_kernel<Rule>, dim3((unsigned)n), dim3(ITEM_THREADS), 0, as_stream(stream), a, rule);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

}  // namespace
}  // namespace sqdet
