// KITTI 2D detection scoring on the GPU: the reference's eval path after the detector (src/eval.py:69-101,
// src/dataset/kitti.py:100-296) without text files or an external evaluator.
//
//   ingest    filter_prediction rows -> the device detection table (det_table.h, KittiRow), each value exactly the double the
//             evaluator's fscanf("%lf") reads back from the detection file kitti_eval.write_detection_files writes
//             (coordinates rounded as '%.2f', scores as '%.3f');
//   evaluate  the KITTI 2D box metric (easy / moderate / hard AP of car, pedestrian, cyclist): per (class, difficulty) a
//             recall pass that collects the scores of the true positives, threshold selection at 41 recall steps, a
//             precision pass with one lane per threshold, then precision = tp / (tp + fp) and its running maximum;
//   analyze   the error analysis of kitti.analyze_detections (correct / localisation / class / background / repeated).
//
// Everything is double precision with -ffp-contract=off (build.py): overlaps, recall steps and the rounding are bitwise
// those of the host programs.  Counts are integer atomics, so results do not depend on scheduling.
#include "det_table.h"   // the table, its ingest ('%.2f' / '%.3f' as the detection files carry them) and the shared helpers

namespace sqdet {
namespace {

constexpr int KMAXD = DT_MAX_ROWS;                  // detection rows per image
constexpr int KMAXG = DT_MAX_GT;                    // ground-truth rows per image
constexpr int NCLASS = 3;                           // car, pedestrian, cyclist
constexpr int NCOMBO = 9;                           // 3 classes x 3 difficulties, combo = class * 3 + difficulty
constexpr int NPTS = 41;                            // recall sample points
constexpr int MAXTHR = 64;                          // threshold slots (<= 41 are ever used; one lane each)
constexpr double NO_DETECTION = -10000000.0;

__constant__ double kMinOverlap[3] = {0.7, 0.5, 0.5};
__constant__ int kMinHeight[3] = {40, 25, 25};
__constant__ int kMaxOcclusion[3] = {0, 1, 2};
__constant__ double kMaxTruncation[3] = {0.15, 0.3, 0.5};

// Workspace of sqdet_kitti_evaluate: a fixed header, then the true-positive scores of every combo.
struct EvalHeader {
  int n_gt[NCOMBO];       // valid ground truth (recall denominator)
  int n_tp[NCOMBO];       // true positives of the recall pass = scores in v
  int n_thr[NCOMBO];      // thresholds selected
  int evaluated[4];       // class detected at least once; [3] unused
  int error;              // a table row over the limits was seen (nothing is scored then)
  int thr_idx[NCOMBO][MAXTHR];
  int pr[NCOMBO][MAXTHR][3];  // tp, fp, fn per threshold
  double thr[NCOMBO][MAXTHR];
  double precision[NCOMBO][NPTS];
  double ap[NCOMBO];
};

// std::max / std::min of the evaluator (the first argument wins ties)
__device__ __forceinline__ double smax(double a, double b) { return (a < b) ? b : a; }
__device__ __forceinline__ double smin(double a, double b) { return (b < a) ? b : a; }

// Overlap of detection a with box b: criterion -1 = intersection over union, 0 = over a's own area.
__device__ __forceinline__ double box_overlap(const double* a, const double* b, int criterion) {
  const double x1 = smax(a[0], b[0]), y1 = smax(a[1], b[1]);
  const double x2 = smin(a[2], b[2]), y2 = smin(a[3], b[3]);
  const double w = x2 - x1, h = y2 - y1;
  if (w <= 0 || h <= 0) return 0;
  const double inter = w * h;
  const double a_area = (a[2] - a[0]) * (a[3] - a[1]);
  if (criterion == 0) return inter / a_area;
  const double b_area = (b[2] - b[0]) * (b[3] - b[1]);
  return inter / (a_area + b_area - inter);
}

// ---------------------------------------------------------------------------------------------------- evaluate
__global__ void __launch_bounds__(64) eval_zero_kernel(int* p, int n) {
  for (int i = threadIdx.x; i < n; i += 64) p[i] = 0;
}

// LDS of one (image, combo) wave: the image's ground truth and the detections of the combo's class.
struct ImageLds {
  double gt[KMAXG][4];
  int ig[KMAXG];       // 0 = valid, 1 = ignored (neighbouring class or over the difficulty), -1 = not of this class
  int dc[KMAXG];       // DontCare rows
  double det[KMAXD][4];
  double score[KMAXD];
  int ngt, nd;
};

// The evaluator's ground truth (sqdet.h): image i owns rows [off[i], off[i + 1]).
struct KittiGt {
  const int32_t* off;
  const double* box;
  const double* trunc;
  const int32_t* occ;
  const int32_t* type;
};

// Loads image `img` for class `c`, difficulty `d`.  Returns false (and flags the error) when a row count is over the limits.
__device__ bool load_image(ImageLds& s, int img, int c, int d, const DetTable& t, const KittiGt& gt, int* error) {
  const int lane = threadIdx.x;
  const int g0 = gt.off[img], ngt = gt.off[img + 1] - g0, nrow = t.count[img];
  if (!rows_ok(ngt, nrow, t.cap)) {
    if (lane == 0) atomicOr(error, 1);
    return false;
  }
  for (int k = lane; k < ngt; k += 64) {
    const double* g = gt.box + (size_t)(g0 + k) * 4;
    for (int q = 0; q < 4; ++q) s.gt[k][q] = g[q];
    const int type = gt.type[g0 + k];
    int valid = -1;
    if (type == c) valid = 1;
    else if ((c == SQDET_KITTI_PEDESTRIAN && type == SQDET_KITTI_PERSON_SITTING) || (c == SQDET_KITTI_CAR && type == SQDET_KITTI_VAN)) valid = 0;
    const double height = g[3] - g[1];
    const bool ignore = gt.occ[g0 + k] > kMaxOcclusion[d] || gt.trunc[g0 + k] > kMaxTruncation[d] || height < kMinHeight[d];
    s.ig[k] = (valid == 1 && !ignore) ? 0 : ((valid == 0 || (ignore && valid == 1)) ? 1 : -1);
    s.dc[k] = type == SQDET_KITTI_DONTCARE;
  }
  const int nd = gather_class_rows(t, img, c, nrow, s.det, s.score);
  if (lane == 0) {
    s.ngt = ngt;
    s.nd = nd;
  }
  __syncthreads();
  return true;
}

// Recall pass (the evaluator's computeStatistics without false positives), one wave per (image, combo): each ground truth
// in order takes the highest-scoring unassigned detection of overlap > MIN_OVERLAP (first index on equal scores).
__global__ void __launch_bounds__(64) eval_recall_kernel(DetTable t, KittiGt gt, int num_gt, EvalHeader* h, double* __restrict__ v) {
  __shared__ ImageLds s;
  __shared__ uint32_t assigned[KMAXD / 32];
  __shared__ double tp_score[KMAXG];
  const int img = blockIdx.x, combo = blockIdx.y, c = combo / 3, d = combo % 3, lane = threadIdx.x;
  if (!load_image(s, img, c, d, t, gt, &h->error)) return;
  const int ngt = s.ngt, nd = s.nd;
  if (lane < KMAXD / 32) assigned[lane] = 0;
  if (lane == 0 && nd > 0) atomicOr(&h->evaluated[c], 1);
  int nvalid = 0, ntp = 0;
  __syncthreads();
  const double min_ov = kMinOverlap[c];
  for (int gi = 0; gi < ngt; ++gi) {
    const int ig = s.ig[gi];
    if (ig == -1) continue;
    nvalid += ig == 0;
    double best = NO_DETECTION;
    int idx = -1;
    for (int j = lane; j < nd; j += 64) {
      if ((assigned[j >> 5] >> (j & 31)) & 1u) continue;
      const double ov = box_overlap(s.det[j], s.gt[gi], -1);
      if (ov > min_ov && s.score[j] > best) {
        best = s.score[j];
        idx = j;
      }
    }
    wave_best_lowest_index(best, idx);  // highest score, lowest index on ties
    if (idx >= 0) {
      if (lane == 0) {
        assigned[idx >> 5] |= 1u << (idx & 31);
        if (ig == 0) tp_score[ntp] = s.score[idx];
      }
      ntp += ig == 0;
    }
    __syncthreads();
  }
  if (lane == 0) {
    if (nvalid) atomicAdd(&h->n_gt[combo], nvalid);
    if (ntp) {
      const int base = atomicAdd(&h->n_tp[combo], ntp);
      for (int k = 0; k < ntp; ++k) v[(size_t)combo * num_gt + base + k] = tp_score[k];
    }
  }
}

// Threshold selection (the evaluator's getThresholds), one wave per combo.  Which sorted positions are taken depends only on
// the number of scores and of valid ground truth: between two picks the running recall target is fixed and "skip i" is
// (r_recall - current) < (current - l_recall), so the wave tests 64 positions at a time and takes the first one not skipped.
__global__ void __launch_bounds__(64) eval_select_kernel(EvalHeader* h) {
  const int combo = blockIdx.x, lane = threadIdx.x;
  const int size = h->n_tp[combo];
  const double n_groundtruth = (double)h->n_gt[combo];
  double current = 0;
  int k = 0, i0 = 0;
  while (i0 < size) {
    int pick = -1;
    for (int base = i0; base < size && pick < 0; base += 64) {
      const int i = base + lane;
      bool take = false;
      if (i < size) {
        const double l_recall = (double)(i + 1) / n_groundtruth;
        const double r_recall = i < size - 1 ? (double)(i + 2) / n_groundtruth : l_recall;
        take = !((r_recall - current) < (current - l_recall) && i < size - 1);
      }
      const uint64_t m = __ballot(take);
      if (m) pick = base + __builtin_ctzll(m);
    }
    if (k < MAXTHR && lane == 0) h->thr_idx[combo][k] = pick;
    ++k;
    current += 1.0 / (NPTS - 1.0);
    i0 = pick + 1;
  }
  if (lane == 0) {
    h->n_thr[combo] = k < MAXTHR ? k : MAXTHR;
    if (k > NPTS) atomicOr(&h->error, 2);
  }
}

// The selected order statistics of the scores (descending): element e sits at sorted positions [#(v > e), #(v >= e)); the
// first copy of a value writes the thresholds that fall there.
__global__ void __launch_bounds__(DT_RANK) eval_rank_kernel(EvalHeader* h, const double* __restrict__ v, int num_gt) {
  __shared__ double tile[DT_RANK];
  const int combo = blockIdx.y, n = h->n_tp[combo], nthr = h->n_thr[combo];
  const int e_idx = blockIdx.x * DT_RANK + threadIdx.x;
  if ((int)(blockIdx.x * DT_RANK) >= n) return;
  const double* vc = v + (size_t)combo * num_gt;
  const double e = e_idx < n ? vc[e_idx] : 0.0;
  const Before b = count_before(vc, n, e, e_idx, tile);
  if (e_idx >= n || b.equal_before) return;
  for (int k = 0; k < nthr; ++k) {
    const int p = h->thr_idx[combo][k];
    if (p >= b.greater && p < b.greater + b.equal) h->thr[combo][k] = e;
  }
}

// Precision pass (computeStatistics with false positives), one wave per (image, combo), lane t = threshold t: detections
// scoring below the threshold are left out, each ground truth takes the unassigned detection of greatest overlap, the rest
// are false positives unless their own area lies in a DontCare region by more than MIN_OVERLAP.
__global__ void __launch_bounds__(64) eval_precision_kernel(DetTable tab, KittiGt gt, EvalHeader* h) {
  __shared__ ImageLds s;
  __shared__ uint32_t assigned[MAXTHR][KMAXD / 32 + 1];
  const int img = blockIdx.x, combo = blockIdx.y, c = combo / 3, d = combo % 3, t = threadIdx.x;
  const int nthr = h->n_thr[combo];
  if (nthr == 0) return;
  if (!load_image(s, img, c, d, tab, gt, &h->error)) return;
  if (t >= nthr) return;
  const int ngt = s.ngt, nd = s.nd;
  uint32_t* a = assigned[t];
  for (int w = 0; w < KMAXD / 32; ++w) a[w] = 0;
  const double thresh = h->thr[combo][t], min_ov = kMinOverlap[c];
  int tp = 0, fp = 0, fn = 0;
  for (int gi = 0; gi < ngt; ++gi) {
    const int ig = s.ig[gi];
    if (ig == -1) continue;
    int idx = -1;
    double max_overlap = 0;
    for (int j = 0; j < nd; ++j) {
      if ((a[j >> 5] >> (j & 31)) & 1u) continue;
      if (s.score[j] < thresh) continue;
      const double ov = box_overlap(s.det[j], s.gt[gi], -1);
      if (ov > min_ov && ov > max_overlap) {
        max_overlap = ov;
        idx = j;
      }
    }
    if (idx < 0) {
      fn += ig == 0;
    } else {
      tp += ig == 0;
      a[idx >> 5] |= 1u << (idx & 31);
    }
  }
  for (int j = 0; j < nd; ++j)
    fp += !((a[j >> 5] >> (j & 31)) & 1u) && !(s.score[j] < thresh);
  for (int gi = 0; gi < ngt; ++gi) {
    if (!s.dc[gi]) continue;
    for (int j = 0; j < nd; ++j) {
      if ((a[j >> 5] >> (j & 31)) & 1u) continue;
      if (s.score[j] < thresh) continue;
      if (box_overlap(s.det[j], s.gt[gi], 0) > min_ov) {
        a[j >> 5] |= 1u << (j & 31);
        --fp;
      }
    }
  }
  if (tp) atomicAdd(&h->pr[combo][t][0], tp);
  if (fp) atomicAdd(&h->pr[combo][t][1], fp);
  if (fn) atomicAdd(&h->pr[combo][t][2], fn);
}

// precision[i] = tp / (tp + fp) (NaN at 0 / 0), then its maximum over [i, 41) as std::max_element finds it -- a NaN at i
// stays, a later NaN never wins, so it is precision[i] or the largest non-NaN value after it -- and AP = the mean of every
// 4th value.  One block per combo: lane i divides, lane 0 scans backwards.
__global__ void __launch_bounds__(64) eval_finish_kernel(EvalHeader* h) {
  __shared__ double p[NPTS];
  const int combo = blockIdx.x, i = threadIdx.x;
  const int nthr = h->n_thr[combo];
  if (i < NPTS) {
    double v = 0;
    if (i < nthr) {
      const int tp = h->pr[combo][i][0], fp = h->pr[combo][i][1];
      v = tp / (double)(tp + fp);
    }
    p[i] = v;
  }
  __syncthreads();
  if (i == 0) {
    bool any = false;
    double suffix = 0;  // largest non-NaN value after the current one
    for (int k = NPTS - 1; k >= 0; --k) {
      const double orig = p[k];
      if (k < nthr && orig == orig && any && orig < suffix) p[k] = suffix;
      if (orig == orig && (!any || suffix < orig)) {
        suffix = orig;
        any = true;
      }
    }
    double ap = 0;
    for (int k = 0; k < NPTS; k += 4) ap += p[k];
    ap /= 11.0;
    h->ap[combo] = ap;
  }
  __syncthreads();
  if (i < NPTS) h->precision[combo][i] = p[i];
}

// ----------------------------------------------------------------------------------------------------- analyze
// kitti.analyze_detections, one wave per image: detections in descending score (stable), the first len(gt) of them
// judged against the image's ground-truth rois by batch_iou (cx, cy, w, h with bbox_transform_inv's +1).
__global__ void __launch_bounds__(64) analyze_kernel(DetTable t, const int32_t* __restrict__ roi_off, const double* __restrict__ roi_box,
                                                     const int32_t* __restrict__ roi_cls, int32_t* __restrict__ counters,
                                                     int32_t* __restrict__ rec_count, int32_t* __restrict__ rec_type,
                                                     int32_t* __restrict__ rec_cls, double* __restrict__ rec_box,
                                                     double* __restrict__ rec_score) {
  __shared__ double det[KMAXD][4];
  __shared__ double score[KMAXD];
  __shared__ int dcls[KMAXD];
  __shared__ int order[KMAXD];
  __shared__ uint8_t detected[KMAXG];
  const int img = blockIdx.x, lane = threadIdx.x;
  const int g0 = roi_off[img], ngt = roi_off[img + 1] - g0, nd = t.count[img];
  if (!rows_ok(ngt, nd, t.cap)) {
    if (lane == 0) {
      atomicOr(&counters[SQDET_KITTI_ANALYSIS_COUNTERS], 1);
      rec_count[img] = 0;
    }
    return;
  }
  const size_t r0 = (size_t)img * t.cap;
  for (int j = lane; j < nd; j += 64) {
    const double* b = t.box + (r0 + j) * 4;
    const double w = b[2] - b[0] + 1.0, hh = b[3] - b[1] + 1.0;
    det[j][0] = b[0] + 0.5 * w;
    det[j][1] = b[1] + 0.5 * hh;
    det[j][2] = w;
    det[j][3] = hh;
    score[j] = t.score[r0 + j];
    dcls[j] = t.cls[r0 + j];
  }
  for (int k = lane; k < ngt; k += 64) detected[k] = 0;
  stable_rank_desc(score, order, nd);
  if (lane != 0) return;
  const size_t rbase = 2 * (size_t)g0;
  int nrec = 0;
  int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // dets, objs, correct, loc, cls, bg, repeated, detected
  cnt[1] = ngt;
  auto record = [&](int type, const double* b, int cl, double sc) {
    const size_t r = rbase + nrec++;
    rec_type[r] = type;
    rec_cls[r] = cl;
    for (int q = 0; q < 4; ++q) rec_box[r * 4 + q] = b[q];
    rec_score[r] = sc;
  };
  if (ngt > 0) {
    const int m = nd < ngt ? nd : ngt;
    cnt[0] = m;
    for (int r = 0; r < m; ++r) {
      const int j = order[r];
      const double* b = det[j];
      double max_iou = 0;
      int gi = -1;
      for (int k = 0; k < ngt; ++k) {
        const double* g = roi_box + (size_t)(g0 + k) * 4;
        double lr = smin(g[0] + 0.5 * g[2], b[0] + 0.5 * b[2]) - smax(g[0] - 0.5 * g[2], b[0] - 0.5 * b[2]);
        double tb = smin(g[1] + 0.5 * g[3], b[1] + 0.5 * b[3]) - smax(g[1] - 0.5 * g[3], b[1] - 0.5 * b[3]);
        lr = smax(lr, 0.0);
        tb = smax(tb, 0.0);
        const double inter = lr * tb;
        const double uni = g[2] * g[3] + b[2] * b[3] - inter;
        const double iou = inter / uni;
        if (gi < 0 || iou > max_iou) {
          max_iou = iou;
          gi = k;
        }
      }
      if (max_iou > 0.1) {
        if (roi_cls[g0 + gi] == dcls[j]) {
          if (max_iou >= 0.5) {
            if (!detected[gi]) {
              ++cnt[2];
              detected[gi] = 1;
            } else {
              ++cnt[6];
            }
          } else {
            ++cnt[3];
            record(SQDET_KITTI_ERR_LOC, b, dcls[j], score[j]);
          }
        } else {
          ++cnt[4];
          record(SQDET_KITTI_ERR_CLS, b, dcls[j], score[j]);
        }
      } else {
        ++cnt[5];
        record(SQDET_KITTI_ERR_BG, b, dcls[j], score[j]);
      }
    }
    for (int k = 0; k < ngt; ++k) {
      if (detected[k]) {
        ++cnt[7];
      } else {
        record(SQDET_KITTI_ERR_MISSED, roi_box + (size_t)(g0 + k) * 4, roi_cls[g0 + k], -1.0);
      }
    }
  }
  rec_count[img] = nrec;
  for (int q = 0; q < 8; ++q)
    if (cnt[q]) atomicAdd(&counters[q], cnt[q]);
}

}  // namespace
}  // namespace sqdet

extern "C" int sqdet_kitti_ingest(const float* boxes, const float* probs, const int32_t* cls, const int32_t* count,
                                  const double* scales, int n, int max_out, double* det_box, double* det_score, int32_t* det_cls,
                                  int32_t* det_count, int32_t* status, int image_offset, int num_images, int cap,
                                  sqdet_stream_t stream) {
  using namespace sqdet;
  return ingest_rows<KittiRow>("kitti_ingest", boxes, probs, cls, count, scales, n, max_out, NCLASS, NCLASS,
                               DetTable{det_box, det_score, det_cls, det_count, status, num_images, cap}, image_offset, stream);
}

extern "C" size_t sqdet_kitti_eval_workspace_bytes(int num_gt) {
  const size_t h = (sizeof(sqdet::EvalHeader) + 255) & ~(size_t)255;
  return h + (size_t)sqdet::NCOMBO * (size_t)(num_gt > 0 ? num_gt : 1) * sizeof(double);
}

extern "C" int sqdet_kitti_evaluate(const double* det_box, const double* det_score, const int32_t* det_cls, const int32_t* det_count,
                                    const int32_t* status, int num_images, int cap, const int32_t* gt_offsets, const double* gt_box,
                                    const double* gt_truncation, const int32_t* gt_occlusion, const int32_t* gt_type, int num_gt,
                                    void* workspace, double* host_precision, double* host_ap, int32_t* host_evaluated,
                                    sqdet_stream_t stream) {
  using namespace sqdet;
  SQDET_REQUIRE(det_box && det_score && det_cls && det_count && gt_offsets && workspace && host_precision && host_ap && host_evaluated,
                "kitti_evaluate: null pointer");
  SQDET_REQUIRE(num_images > 0 && cap > 0 && num_gt >= 0, "kitti_evaluate: bad dims");
  SQDET_REQUIRE(num_gt == 0 || (gt_box && gt_truncation && gt_occlusion && gt_type), "kitti_evaluate: null ground-truth pointer");
  SQDET_UNSUPPORTED(cap > SQDET_KITTI_MAX_DETECTIONS, "kitti_evaluate: %d rows per image (limit %d)", cap, SQDET_KITTI_MAX_DETECTIONS);
  hipStream_t st = as_stream(stream);
  const DetTable t = read_only_table(det_box, det_score, det_cls, det_count, status, num_images, cap);
  const KittiGt gt = {gt_offsets, gt_box, gt_truncation, gt_occlusion, gt_type};
  EvalHeader* h = reinterpret_cast<EvalHeader*>(workspace);
  double* v = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + ((sizeof(EvalHeader) + 255) & ~(size_t)255));
  const int ng = num_gt > 0 ? num_gt : 1;
  hipLaunchKernelGGL(eval_zero_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<int*>(h),
                     (int)(offsetof(EvalHeader, thr) / sizeof(int)));
  hipLaunchKernelGGL(eval_recall_kernel, dim3((unsigned)num_images, NCOMBO), dim3(64), 0, st, t, gt, ng, h, v);
  hipLaunchKernelGGL(eval_select_kernel, dim3(NCOMBO), dim3(64), 0, st, h);
  hipLaunchKernelGGL(eval_rank_kernel, dim3((unsigned)((ng + DT_RANK - 1) / DT_RANK), NCOMBO), dim3(DT_RANK), 0, st, h, v, ng);
  hipLaunchKernelGGL(eval_precision_kernel, dim3((unsigned)num_images, NCOMBO), dim3(64), 0, st, t, gt, h);
  hipLaunchKernelGGL(eval_finish_kernel, dim3(NCOMBO), dim3(64), 0, st, h);
  SQDET_CHECK_HIP(hipGetLastError());
  EvalHeader host;
  if (const int rc = read_back("kitti_evaluate", h, t, NCLASS, st, &host)) return rc;
  SQDET_REQUIRE(!(host.error & 2), "kitti_evaluate: more than 41 recall thresholds");
  for (int c = 0; c < NCOMBO; ++c) {
    for (int i = 0; i < NPTS; ++i) host_precision[c * NPTS + i] = host.precision[c][i];
    host_ap[c] = host.ap[c];
  }
  for (int c = 0; c < 3; ++c) host_evaluated[c] = host.evaluated[c];
  return SQDET_OK;
}

extern "C" int sqdet_kitti_analyze(const double* det_box, const double* det_score, const int32_t* det_cls, const int32_t* det_count,
                                   int num_images, int cap, const int32_t* roi_offsets, const double* roi_box, const int32_t* roi_cls,
                                   int num_rois, int32_t* counters, int32_t* rec_count, int32_t* rec_type, int32_t* rec_cls,
                                   double* rec_box, double* rec_score, sqdet_stream_t stream) {
  using namespace sqdet;
  SQDET_REQUIRE(det_box && det_score && det_cls && det_count && roi_offsets && counters && rec_count, "kitti_analyze: null pointer");
  SQDET_REQUIRE(num_images > 0 && cap > 0 && num_rois >= 0, "kitti_analyze: bad dims");
  SQDET_REQUIRE(num_rois == 0 || (roi_box && roi_cls && rec_type && rec_cls && rec_box && rec_score),
                "kitti_analyze: null roi / record pointer");
  SQDET_UNSUPPORTED(cap > SQDET_KITTI_MAX_DETECTIONS, "kitti_analyze: %d rows per image (limit %d)", cap, SQDET_KITTI_MAX_DETECTIONS);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(eval_zero_kernel, dim3(1), dim3(64), 0, st, counters, SQDET_KITTI_ANALYSIS_COUNTERS + 1);
  hipLaunchKernelGGL(analyze_kernel, dim3((unsigned)num_images), dim3(64), 0, st,
                     read_only_table(det_box, det_score, det_cls, det_count, nullptr, num_images, cap), roi_offsets, roi_box, roi_cls,
                     counters, rec_count, rec_type, rec_cls, rec_box, rec_score);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}
