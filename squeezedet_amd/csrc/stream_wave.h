// What a kernel with one WAVE per stream uses (track.hip, mot_eval.hip): lane r is row r of a frame of at most 64 rows, sets of
// rows are 64-bit ballot masks uniform over the wave, and the pairs of two such sets are dealt to the 64 lanes in turn.
// Build with -ffp-contract=off: iou() is util.iou operation for operation, compared bit for bit with the NumPy restatements.
#pragma once
#include "common.h"

namespace sqdet {
namespace {

__device__ __forceinline__ double dmin(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double dmax(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ bool finite_f(float v) { return __builtin_fabsf(v) < __builtin_inff(); }      // false for NaN
__device__ __forceinline__ bool finite_d(double v) { return __builtin_fabs(v) < __builtin_inf(); }
__device__ __forceinline__ uint64_t below(int lane) { return (1ull << lane) - 1ull; }
// The number of lanes of `mask` below `lane`: its rank in the set.
__device__ __forceinline__ int rank_in(uint64_t mask, int lane) { return __popcll(mask & below(lane)); }

// util.iou (utils/util.py:9-30) of two boxes (cx, cy, w, h)
__device__ __forceinline__ double iou(const double a[4], const double b[4]) {
  const double lr = dmin(a[0] + 0.5 * a[2], b[0] + 0.5 * b[2]) - dmax(a[0] - 0.5 * a[2], b[0] - 0.5 * b[2]);
  if (!(lr > 0.0)) return 0.0;
  const double tb = dmin(a[1] + 0.5 * a[3], b[1] + 0.5 * b[3]) - dmax(a[1] - 0.5 * a[3], b[1] - 0.5 * b[3]);
  if (!(tb > 0.0)) return 0.0;
  const double inter = lr * tb;
  return inter / (a[2] * a[3] + b[2] * b[3] - inter);
}

// A count the caller wrote, kept inside the `rows` there are.
__device__ __forceinline__ int clamp_count(int c, int rows) { return c < 0 ? 0 : (c > rows ? rows : c); }

// A row (cx, cy, w, h) that can be matched: four finite values, w > 0, h > 0.
__device__ __forceinline__ bool valid_box(const f32x4& b) {
  return finite_f(b[0]) && finite_f(b[1]) && finite_f(b[2]) && finite_f(b[3]) && b[2] > 0.0f && b[3] > 0.0f;
}
__device__ __forceinline__ bool valid_box(const double b[4]) {
  return finite_d(b[0]) && finite_d(b[1]) && finite_d(b[2]) && finite_d(b[3]) && b[2] > 0.0 && b[3] > 0.0;
}

// The lanes of `mask` as an ordered LDS list: a lane of the set (mine: its bit) writes itself at its rank.
__device__ __forceinline__ void list_lane(bool mine, uint64_t mask, int* list, int lane) {
  if (mine) list[rank_in(mask, lane)] = lane;
}

// body(a, b) for every pair of list_a[0 .. n_a) x list_b[0 .. n_b), a-major, the pairs dealt to the 64 lanes in turn.
template <class Body>
__device__ __forceinline__ void deal_pairs(int n_a, int n_b, const int* list_a, const int* list_b, int lane, Body body) {
  for (int q = lane; q < n_a * n_b; q += 64) {
    const int i = q / n_b;
    body(list_a[i], list_b[q - i * n_b]);
  }
}

// One workgroup per stream, or max_workgroups (> 0) that walk the streams.
inline int stream_grid(int max_workgroups, int streams) { return max_workgroups > 0 && max_workgroups < streams ? max_workgroups : streams; }

}  // namespace
}  // namespace sqdet
