// What labels.hip (sqdet_build_labels) and assign.hip (sqdet_build_labels_opt) share: the candidate order and its workgroup
// reduction, batch_iou's float64 expression, and the launcher of the reference's assignment (labels.hip's three kernels).
// Both files are compiled with -ffp-contract=off: every expression here is one IEEE operation per operator, as NumPy evaluates it.
#pragma once
#include "common.h"

namespace sqdet {

struct Cand {
  double v;
  int idx;
};

// better(a, b): a wins over b.  MAXMODE: larger v, ties -> higher idx.  else: smaller v, ties -> lower idx.
template <bool MAXMODE>
__device__ __forceinline__ bool better(const Cand& a, const Cand& b) {
  if (a.idx < 0) return false;
  if (b.idx < 0) return true;
  if (MAXMODE) return a.v > b.v || (a.v == b.v && a.idx > b.idx);
  return a.v < b.v || (a.v == b.v && a.idx < b.idx);
}

template <bool MAXMODE>
__device__ __forceinline__ Cand block_best(Cand c, Cand* red) {
  // wave reduction, then one candidate per wave through LDS
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Cand o;
    o.v = __shfl_down(c.v, off);
    o.idx = __shfl_down(c.idx, off);
    if (better<MAXMODE>(o, c)) c = o;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                       // red[] free (previous use finished)
  if (lane == 0) red[wave] = c;
  __syncthreads();
  Cand b = red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
    if (better<MAXMODE>(red[w], b)) b = red[w];
  return b;
}

// A ground-truth box (cx, cy, w, h) with the edges and the area batch_iou (utils/util.py:32-54) forms from it.
struct GtBox {
  double gx, gy, gw, gh, gl, gr, gtp, gb, garea;
};

__device__ __forceinline__ GtBox gt_box(const double* g) {
  GtBox q;
  q.gx = g[0]; q.gy = g[1]; q.gw = g[2]; q.gh = g[3];
  q.gl = q.gx - 0.5 * q.gw; q.gr = q.gx + 0.5 * q.gw; q.gtp = q.gy - 0.5 * q.gh; q.gb = q.gy + 0.5 * q.gh;
  q.garea = q.gw * q.gh;
  return q;
}

// batch_iou's intersection area and the IoU from it, float64, in the reference's operation order
__device__ __forceinline__ double anchor_inter(const GtBox& q, double ax, double ay, double aw, double ah) {
  double lr = fmin(ax + 0.5 * aw, q.gr) - fmax(ax - 0.5 * aw, q.gl);
  lr = lr > 0.0 ? lr : 0.0;
  double tb = fmin(ay + 0.5 * ah, q.gb) - fmax(ay - 0.5 * ah, q.gtp);
  tb = tb > 0.0 ? tb : 0.0;
  return lr * tb;
}

__device__ __forceinline__ double iou_from_inter(const GtBox& q, double inter, double aw, double ah) {
  return inter / (aw * ah + q.garea - inter);
}

// The dense rows of a positive anchor (train.py:163-224): mask, delta in float64 rounded once, the box, the one-hot class.
__device__ __forceinline__ void write_positive_rows(const GtBox& q, double ax, double ay, double aw, double ah, int cls, int a, int C,
                                                    float* __restrict__ m, float* __restrict__ d, float* __restrict__ bx,
                                                    float* __restrict__ lb) {
  m[a] = 1.f;
  d[a * 4 + 0] = (float)((q.gx - ax) / aw);
  d[a * 4 + 1] = (float)((q.gy - ay) / ah);
  d[a * 4 + 2] = (float)log(q.gw / aw);
  d[a * 4 + 3] = (float)log(q.gh / ah);
  bx[a * 4 + 0] = (float)q.gx; bx[a * 4 + 1] = (float)q.gy; bx[a * 4 + 2] = (float)q.gw; bx[a * 4 + 3] = (float)q.gh;
  if (cls >= 0 && cls < C) lb[a * C + cls] = 1.f;
}

// labels.hip: sqdet_build_labels' argument checks (an error code, nothing launched) and its three launches.
int labels_check_args(const void* anchors_f64, const void* gt_boxes_f64, const void* gt_classes, const void* gt_counts,
                      const void* input_mask, const void* box_delta_input, const void* box_input, const void* labels,
                      const void* anchor_index, int batch, int num_anchors, int max_objects, int classes);
void labels_launch_reference(const double* anchors_f64, const double* gt_boxes_f64, const int* gt_classes, const int* gt_counts,
                             float* input_mask, float* box_delta_input, float* box_input, float* labels, int* anchor_index,
                             int batch, int num_anchors, int max_objects, int classes, hipStream_t st);

}  // namespace sqdet
