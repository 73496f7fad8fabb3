// More than one positive anchor per ground-truth box (OURS): sqdet_build_labels_opt.  The reference
// (imdb.py:195-239) trains exactly one anchor per object; here every object keeps that anchor and may get more of the anchors
// no object claimed, by one of two rules:
//   iou   every anchor with IoU >= iou_thresh, at most the max_per_box best of the box (larger IoU, ties -> higher index);
//   atss  Zhang et al., CVPR 2020: per anchor shape the topk anchors nearest the box centre are the candidates; the threshold
//         is mean + std of their IoUs (tested without a square root: e = iou - mean >= 0 and e * e >= var); a positive's
//         centre lies strictly inside the box.
// An anchor eligible for several boxes goes to the box of largest IoU, ties to the lower box.
//
// Five launches: labels.hip's three (zero, best, resolve -- the claimed anchors and their rows, bit for bit sqdet_build_labels),
// then
//   4. assign_describe_kernel, one workgroup per (image, box): the box's descriptor into the workspace -- iou: the K-th element
//      (iou_K, idx_K) of the box's order; atss: per shape the k-th nearest (d_k, idx_k), then the mean and the population
//      variance of the candidates' IoUs.  What a selection compares is staged in LDS once (the anchors at or above the
//      threshold; the distances of one shape's cells), then K rounds of block_best pick the best element strictly behind the
//      previous pick -- no exclusion set.  The atss picks are kept in LDS, ranked by index in parallel and summed by ONE thread
//      in ascending index.  It also clears positives[b, i];
//   5. assign_anchor_kernel, one thread per (image, anchor): over the image's boxes, the claim (anchor_index) or the eligible
//      box of largest IoU, tested against the descriptors with an (iou, idx) / (d, idx) comparison; writes assigned_box, the
//      rows of an unclaimed positive, and counts with an integer atomicAdd (no float atomics: the counts are exact in any order).
// No memset node, no host synchronisation, no allocation: capturable in a hipGraph like sqdet_build_labels.
#include "labels_common.h"

namespace sqdet {

enum { ASSIGN_IOU = 1, ASSIGN_ATSS = 2, ASSIGN_MAX_PER_BOX = 64, ASSIGN_MAX_TOPK = 32, ASSIGN_MAX_CANDIDATES = 1024, ASSIGN_STAGE_CAP = 4096 };

// workspace: doubles first (8-byte aligned), then ints.  iou: per box 1 double (iou_K) + 1 int (idx_K);
// atss: per box 2 + apg doubles (mean, var, d_k per shape) + apg ints (idx_k per shape).
__host__ __device__ inline size_t ws_doubles_per_box(int mode, int apg) { return mode == ASSIGN_IOU ? 1 : 2 + (size_t)apg; }
__host__ __device__ inline size_t ws_ints_per_box(int mode, int apg) { return mode == ASSIGN_IOU ? 1 : (size_t)apg; }

__device__ __forceinline__ double centre_dist(const GtBox& q, double ax, double ay) {
  const double d0 = q.gx - ax, d1 = q.gy - ay;
  return d0 * d0 + d1 * d1;
}

// One anchor row (cx, cy, w, h) as two 16-byte loads.
struct AnchorRow {
  double ax, ay, aw, ah;
};

__device__ __forceinline__ AnchorRow load_anchor(const double* __restrict__ anchors, int a) {
  const double2 lo = *reinterpret_cast<const double2*>(anchors + (size_t)a * 4);
  const double2 hi = *reinterpret_cast<const double2*>(anchors + (size_t)a * 4 + 2);
  AnchorRow r;
  r.ax = lo.x; r.ay = lo.y; r.aw = hi.x; r.ah = hi.y;
  return r;
}

// K rounds of block_best over `count` staged values: round r picks the best element strictly behind round r - 1's pick.
// implicit_base >= 0: element t is anchor implicit_base + t * stride (atss: the cells of one shape); else its index is idx[t].
// Returns the last pick ((0, -1): fewer than K elements) and, through `on_pick`, every pick in order.  Workgroup-uniform.
template <bool MAXMODE, typename F>
__device__ __forceinline__ Cand staged_rounds(const double* val, const int* idx, int implicit_base, int stride, int count, int K,
                                              Cand* red, bool all_or_nothing, F on_pick) {
  Cand prev;
  prev.v = 0.0; prev.idx = -1;
  for (int r = 0; r < K; ++r) {
    Cand c;
    c.v = 0.0; c.idx = -1;
    for (int t = threadIdx.x; t < count; t += blockDim.x) {
      Cand q;
      q.v = val[t]; q.idx = implicit_base >= 0 ? implicit_base + t * stride : idx[t];
      if ((r == 0 || better<MAXMODE>(prev, q)) && better<MAXMODE>(q, c)) c = q;
    }
    const Cand best = block_best<MAXMODE>(c, red);
    if (best.idx < 0) {                              // fewer than K elements
      if (all_or_nothing) { prev.v = 0.0; prev.idx = -1; }
      break;
    }
    prev = best;
    on_pick(best);
  }
  return prev;
}

// One workgroup per (image, box).  The values a round compares are staged in LDS once -- iou: the (iou, index) of the
// anchors with IoU > 0 and >= iou_thresh, appended in any order (the rounds select by the total order, not by position); atss: the squared
// distance of every cell of the current shape -- so a round reads LDS, not 32-byte rows at L2 latency.  A box with more than
// ASSIGN_STAGE_CAP overlapping anchors, or a table with more cells than that, takes the same rounds over global memory.
__global__ __launch_bounds__(256) void assign_describe_kernel(const double* __restrict__ anchors, const double* __restrict__ gt,
                                                               const int* __restrict__ gt_count, int* __restrict__ positives,
                                                               double* __restrict__ ws_d, int* __restrict__ ws_i, int A, int M,
                                                               int apg, int mode, int K, double thresh) {
  __shared__ Cand red[16];
  __shared__ double stage_v[ASSIGN_STAGE_CAP];
  __shared__ int stage_i[ASSIGN_STAGE_CAP];
  __shared__ int mem_idx[ASSIGN_MAX_CANDIDATES];
  __shared__ double srt_iou[ASSIGN_MAX_CANDIDATES];
  __shared__ int staged;
  const int i = blockIdx.x, b = blockIdx.y;
  const size_t bi = (size_t)b * M + i;
  if (threadIdx.x == 0) positives[bi] = 0;
  int n = gt_count[b];
  if (n > M) n = M;
  if (i >= n) return;                                // (its descriptor is never read)
  const GtBox q = gt_box(gt + bi * 4);
  double* wd = ws_d + bi * ws_doubles_per_box(mode, apg);
  int* wi = ws_i + bi * ws_ints_per_box(mode, apg);
  if (mode == ASSIGN_IOU) {
    if (threadIdx.x == 0) staged = 0;
    __syncthreads();
    for (int a = threadIdx.x; a < A; a += blockDim.x) {
      const AnchorRow r = load_anchor(anchors, a);
      const double inter = anchor_inter(q, r.ax, r.ay, r.aw, r.ah);
      if (!(inter > 0.0)) continue;                  // 0 / union is 0 or NaN: never > 0 (spares the float64 division)
      const double iou = iou_from_inter(q, inter, r.aw, r.ah);
      if (!(iou > 0.0) || !(iou >= thresh)) continue;    // (the anchors >= thresh head the order: its first K are theirs)
      const int pos = atomicAdd(&staged, 1);         // (an LDS counter: the order of the list does not matter)
      if (pos < ASSIGN_STAGE_CAP) {
        stage_v[pos] = iou;
        stage_i[pos] = a;
      }
    }
    __syncthreads();
    const int count = staged;
    Cand last;
    if (count <= ASSIGN_STAGE_CAP) {
      last = staged_rounds<true>(stage_v, stage_i, -1, 0, count, K, red, true, [](const Cand&) {});
    } else {                                         // too many overlaps to stage: the same rounds over the table
      last.v = 0.0; last.idx = -1;
      for (int r = 0; r < K; ++r) {
        Cand c;
        c.v = 0.0; c.idx = -1;
        for (int a = threadIdx.x; a < A; a += blockDim.x) {
          const AnchorRow w = load_anchor(anchors, a);
          const double inter = anchor_inter(q, w.ax, w.ay, w.aw, w.ah);
          if (!(inter > 0.0)) continue;
          Cand t;
          t.v = iou_from_inter(q, inter, w.aw, w.ah); t.idx = a;
          if (t.v > 0.0 && t.v >= thresh && (r == 0 || better<true>(last, t)) && better<true>(t, c)) c = t;
        }
        const Cand best = block_best<true>(c, red);
        if (best.idx < 0) {                          // the order has fewer than K elements (workgroup-uniform)
          last.v = 0.0; last.idx = -1;
          break;
        }
        last = best;
      }
    }
    if (threadIdx.x == 0) {                          // fewer than K anchors reach the threshold: (0, -1), each of them passes
      wd[0] = last.v;
      wi[0] = last.idx;
    }
    return;
  }
  // atss
  const int cells = A / apg;
  int count = 0;                                     // workgroup-uniform: block_best hands every thread the pick
  for (int s = 0; s < apg; ++s) {
    Cand last;
    auto keep = [&](const Cand& pick) {
      if (threadIdx.x == 0) mem_idx[count] = pick.idx;
      ++count;                                       // <= apg * min(K, cells) <= ASSIGN_MAX_CANDIDATES (checked by the entry)
    };
    if (cells <= ASSIGN_STAGE_CAP) {
      __syncthreads();                               // the previous shape's rounds have read stage_v
      for (int cell = threadIdx.x; cell < cells; cell += blockDim.x) {
        const int a = cell * apg + s;
        const double2 c = *reinterpret_cast<const double2*>(anchors + (size_t)a * 4);
        stage_v[cell] = centre_dist(q, c.x, c.y);
      }
      __syncthreads();
      last = staged_rounds<false>(stage_v, stage_i, s, apg, cells, K, red, false, keep);
    } else {
      last.v = 0.0; last.idx = -1;
      for (int r = 0; r < K; ++r) {
        Cand c;
        c.v = 0.0; c.idx = -1;
        for (int cell = threadIdx.x; cell < cells; cell += blockDim.x) {
          const int a = cell * apg + s;
          Cand t;
          t.v = centre_dist(q, anchors[(size_t)a * 4], anchors[(size_t)a * 4 + 1]); t.idx = a;
          if ((r == 0 || better<false>(last, t)) && better<false>(t, c)) c = t;
        }
        const Cand best = block_best<false>(c, red);
        if (best.idx < 0) break;                     // the shape has fewer than K anchors: all of them are taken
        last = best;
        keep(best);
      }
    }
    if (threadIdx.x == 0) {
      wd[2 + s] = last.v;
      wi[s] = last.idx;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < count; t += blockDim.x) {
    const int a = mem_idx[t];
    int rank = 0;
    for (int u = 0; u < count; ++u) rank += mem_idx[u] < a;      // (the picks are distinct anchors)
    const AnchorRow r = load_anchor(anchors, a);
    srt_iou[rank] = iou_from_inter(q, anchor_inter(q, r.ax, r.ay, r.aw, r.ah), r.aw, r.ah);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int t = 0; t < count; ++t) sum = sum + srt_iou[t];
    const double mean = sum / (double)count;
    double sq = 0.0;
    for (int t = 0; t < count; ++t) {
      const double e = srt_iou[t] - mean;
      sq = sq + e * e;
    }
    wd[0] = mean;
    wd[1] = sq / (double)count;
  }
}

__global__ __launch_bounds__(256) void assign_anchor_kernel(const double* __restrict__ anchors, const double* __restrict__ gt,
                                                            const int* __restrict__ gt_cls, const int* __restrict__ gt_count,
                                                            const int* __restrict__ aidx, const double* __restrict__ ws_d,
                                                            const int* __restrict__ ws_i, float* __restrict__ mask,
                                                            float* __restrict__ delta, float* __restrict__ box,
                                                            float* __restrict__ labels, int* __restrict__ assigned_box,
                                                            int* __restrict__ positives, int A, int M, int C, int apg, int mode,
                                                            double thresh) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (a >= A) return;
  int n = gt_count[b];
  if (n > M) n = M;
  // one 32-byte row per thread, consecutive threads consecutive rows
  const AnchorRow row = load_anchor(anchors, a);
  const double ax = row.ax, ay = row.ay, aw = row.aw, ah = row.ah;
  const int shape = mode == ASSIGN_ATSS ? a % apg : 0;
  const size_t nd = ws_doubles_per_box(mode, apg), ni = ws_ints_per_box(mode, apg);
  int claimed = -1, won = -1;
  double won_iou = 0.0;
  for (int i = 0; i < n; ++i) {
    const size_t bi = (size_t)b * M + i;
    if (aidx[bi] == a) {
      claimed = i;
      break;                                         // (one owner per anchor: labels_resolve_kernel's claimed set)
    }
    const GtBox q = gt_box(gt + bi * 4);
    const double inter = anchor_inter(q, ax, ay, aw, ah);
    if (!(inter > 0.0)) continue;
    const double iou = iou_from_inter(q, inter, aw, ah);
    if (!(iou > 0.0) || !(iou > won_iou)) continue;  // not eligible, or loses to an earlier box (ties -> lower box)
    const double* wd = ws_d + bi * nd;
    const int* wi = ws_i + bi * ni;
    bool ok;
    if (mode == ASSIGN_IOU) {
      const double vk = wd[0];
      ok = iou >= thresh && (iou > vk || (iou == vk && a >= wi[0]));
    } else {
      const double d = centre_dist(q, ax, ay), dk = wd[2 + shape];
      const double e = iou - wd[0];
      ok = (d < dk || (d == dk && a <= wi[shape])) && e >= 0.0 && e * e >= wd[1] && q.gl < ax && ax < q.gr && q.gtp < ay && ay < q.gb;
    }
    if (ok) {
      won = i;
      won_iou = iou;
    }
  }
  const int owner = claimed >= 0 ? claimed : won;
  assigned_box[(size_t)b * A + a] = owner;
  if (owner < 0) return;
  atomicAdd(positives + (size_t)b * M + owner, 1);
  if (claimed < 0) {                                 // (a claimed anchor's rows are labels_resolve_kernel's)
    const size_t bi = (size_t)b * M + owner;
    write_positive_rows(gt_box(gt + bi * 4), ax, ay, aw, ah, gt_cls[bi], a, C, mask + (size_t)b * A, delta + (size_t)b * A * 4,
                        box + (size_t)b * A * 4, labels + (size_t)b * A * C);
  }
}

static int assign_check_options(int num_anchors, int anchors_per_grid, const sqdet_assign_options_t* opt) {
  SQDET_REQUIRE(opt, "build_labels_opt: null options");
  SQDET_REQUIRE(opt->mode == ASSIGN_IOU || opt->mode == ASSIGN_ATSS, "build_labels_opt: mode %d is neither 1 (iou) nor 2 (atss)", opt->mode);
  SQDET_REQUIRE(num_anchors > 0 && anchors_per_grid > 0, "build_labels_opt: bad dims");
  SQDET_REQUIRE(num_anchors % anchors_per_grid == 0, "build_labels_opt: %d anchors are no multiple of anchors_per_grid %d", num_anchors,
                anchors_per_grid);
  if (opt->mode == ASSIGN_IOU) {
    SQDET_REQUIRE(opt->iou_thresh >= 0.0, "build_labels_opt: iou_thresh must be >= 0");
    SQDET_REQUIRE(opt->max_per_box >= 1, "build_labels_opt: max_per_box must be >= 1");
    SQDET_UNSUPPORTED(opt->max_per_box > ASSIGN_MAX_PER_BOX, "build_labels_opt: max_per_box %d > %d", opt->max_per_box, ASSIGN_MAX_PER_BOX);
  } else {
    SQDET_REQUIRE(opt->topk >= 1, "build_labels_opt: topk must be >= 1");
    SQDET_UNSUPPORTED(opt->topk > ASSIGN_MAX_TOPK, "build_labels_opt: topk %d > %d", opt->topk, ASSIGN_MAX_TOPK);
    const long cells = num_anchors / anchors_per_grid;
    const long cand = (long)anchors_per_grid * (opt->topk < cells ? opt->topk : cells);
    SQDET_UNSUPPORTED(cand > ASSIGN_MAX_CANDIDATES, "build_labels_opt: %ld atss candidates per box (anchors_per_grid x topk) > %d", cand,
                      ASSIGN_MAX_CANDIDATES);
  }
  return SQDET_OK;
}

}  // namespace sqdet

extern "C" size_t sqdet_build_labels_opt_workspace_bytes(int batch, int num_anchors, int max_objects, int anchors_per_grid,
                                                         const sqdet_assign_options_t* opt) {
  using namespace sqdet;
  if (batch <= 0 || max_objects <= 0 || assign_check_options(num_anchors, anchors_per_grid, opt) != SQDET_OK) return 0;
  const size_t boxes = (size_t)batch * max_objects;
  const size_t bytes = boxes * ws_doubles_per_box(opt->mode, anchors_per_grid) * 8 + boxes * ws_ints_per_box(opt->mode, anchors_per_grid) * 4;
  return (bytes + 7) / 8 * 8;
}

extern "C" int sqdet_build_labels_opt(const double* anchors_f64, const double* gt_boxes_f64, const int* gt_classes,
                                      const int* gt_counts, float* input_mask, float* box_delta_input, float* box_input,
                                      float* labels, int* anchor_index, int* assigned_box, int* positives, void* workspace,
                                      int batch, int num_anchors, int max_objects, int classes, int anchors_per_grid,
                                      const sqdet_assign_options_t* opt, sqdet_stream_t stream) {
  using namespace sqdet;
  int rc = labels_check_args(anchors_f64, gt_boxes_f64, gt_classes, gt_counts, input_mask, box_delta_input, box_input, labels,
                             anchor_index, batch, num_anchors, max_objects, classes);
  if (rc != SQDET_OK) return rc;
  SQDET_REQUIRE(assigned_box && positives && workspace, "build_labels_opt: null pointer");
  SQDET_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)anchors_f64 & 15) == 0, "build_labels_opt: workspace must be 8-byte, anchors 16-byte aligned");
  rc = assign_check_options(num_anchors, anchors_per_grid, opt);
  if (rc != SQDET_OK) return rc;
  hipStream_t st = as_stream(stream);
  labels_launch_reference(anchors_f64, gt_boxes_f64, gt_classes, gt_counts, input_mask, box_delta_input, box_input, labels,
                          anchor_index, batch, num_anchors, max_objects, classes, st);
  const int mode = opt->mode, K = mode == ASSIGN_IOU ? opt->max_per_box : opt->topk;
  double* ws_d = static_cast<double*>(workspace);
  int* ws_i = reinterpret_cast<int*>(ws_d + (size_t)batch * max_objects * ws_doubles_per_box(mode, anchors_per_grid));
  hipLaunchKernelGGL(assign_describe_kernel, dim3((unsigned)max_objects, (unsigned)batch), dim3(256), 0, st, anchors_f64, gt_boxes_f64,
                     gt_counts, positives, ws_d, ws_i, num_anchors, max_objects, anchors_per_grid, mode, K, opt->iou_thresh);
  hipLaunchKernelGGL(assign_anchor_kernel, dim3((unsigned)((num_anchors + 255) / 256), (unsigned)batch), dim3(256), 0, st, anchors_f64,
                     gt_boxes_f64, gt_classes, gt_counts, anchor_index, ws_d, ws_i, input_mask, box_delta_input, box_input, labels,
                     assigned_box, positives, num_anchors, max_objects, classes, anchors_per_grid, mode, opt->iou_thresh);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}
