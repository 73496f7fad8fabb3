// COCO-style detection scoring on the GPU: the published COCOeval bbox protocol -- average precision over IoU 0.50:0.05:0.95
// and average recall at 1 / 10 / 100 detections, by object size -- on the device detection table, for every class, IoU
// threshold, area range and detection limit at once.
//
//   ingest    filter_prediction rows -> the table (det_table.h, CocoRow): x, y, w, h and the score as doubles, nothing rounded;
//   evaluate  count (kept rows per (image, class), non-ignored objects per (class, area range)), scan (where each (image,
//             class) segment starts in its class's list), match (one wave per (image, class): the greedy walk, every
//             threshold and area range), rank (each row's position in its class's order) and accumulate (one block per
//             (class, area range, detection limit, threshold): tp / fp prefix sums, recall, the precision envelope and its
//             value at every recall threshold).
//
// Everything is double precision with -ffp-contract=off (build.py); every floating-point value is one rounded IEEE operation
// on integers or table values in a fixed order and the sums are integer, so the arrays are reproducible bit for bit.  The
// IoU, recall and area thresholds come from the host as it computes them (np.linspace): none is recomputed here.
#include <string.h>

#include <vector>

#include "det_table.h"

namespace sqdet {
namespace {

constexpr int CMAXD = DT_MAX_ROWS;                 // detection rows per image
constexpr int CMAXG = DT_MAX_GT;                   // ground-truth rows per image
constexpr int CMAXC = SQDET_COCO_MAX_CLASSES;
constexpr int CMAXT = SQDET_COCO_MAX_IOU_THRESHOLDS;
constexpr int CMAXA = SQDET_COCO_MAX_AREA_RANGES;
constexpr int CMAXM = SQDET_COCO_MAX_DET_LIMITS;
constexpr int CMAXK = SQDET_COCO_MAX_KEPT;         // the largest detection limit: rows kept per (image, class)
constexpr int SCAN = DT_RANK;
static_assert(CMAXG == 2 * 64, "the matcher holds an image's objects two to a lane");
static_assert(2 * CMAXT <= 32, "a row's matched and ignored bits of one area range share a 32-bit word");
enum { GT_IGNORE = 1, GT_CROWD = 2 };

struct CocoHeader {
  int error;  // an image over the row limits was seen (it is scored as empty; the call fails)
  int pad;
  int ndet[CMAXC];          // kept rows of the class
  int npig[CMAXC * CMAXA];  // [class, area range] objects that are not ignored
};

struct CocoLists {  // the host's threshold lists, copied to the device as they are
  double iou[CMAXT], rec[SQDET_COCO_MAX_RECALL_THRESHOLDS], area[2 * CMAXA];
  int32_t max_det[CMAXM + 1];
};
static_assert(sizeof(CocoLists) % 8 == 0, "no padding at its end");

struct CocoParams {  // where the kernels read them
  const double* iou_thr;   // [T]
  const double* rec_thr;   // [R]
  const double* area_rng;  // [A, 2] lo, hi (both inclusive)
  const int32_t* max_det;  // [M] ascending
  int T, R, A, M;
};

// The workspace of sqdet_coco_evaluate; the per-row arrays hold the class lists of det_table.h, each segment's rows by rank.
struct CocoWorkspace {
  CocoHeader* h;
  double* precision;  // [T, R, K, A, M]
  double* recall;     // [T, K, A, M]
  double* cscore;     // [rows] score, class lists
  int* cnt_det;       // [K, N] kept rows of the class in the image
  int* base;          // [K, N] exclusive prefix of cnt_det over the images
  int* crank;         // [rows] rank in the image, class lists
  int* cword;         // [A, rows] matched / ignored bits, class lists
  CocoLists* lists;
  size_t out_bytes;   // header + precision + recall: what goes back to the host
  size_t bytes;
};

CocoWorkspace carve(void* p, int num_images, int cap, int classes, int T, int R, int A, int M) {
  const size_t rows = (size_t)num_images * cap, KN = (size_t)classes * num_images;
  Carver k{reinterpret_cast<char*>(p)};
  CocoWorkspace w;
  w.h = k.take<CocoHeader>(1);
  w.precision = k.take<double>((size_t)T * R * classes * A * M, 256);
  w.recall = k.take<double>((size_t)T * classes * A * M);
  w.out_bytes = k.o;
  w.cscore = k.take<double>(rows);
  w.cnt_det = k.take<int>(KN);
  w.base = k.take<int>(KN);
  w.crank = k.take<int>(rows);
  w.cword = k.take<int>((size_t)A * rows);
  w.lists = k.take<CocoLists>(1);
  w.bytes = k.o;
  return w;
}

// Is the object ignored in the area range [lo, hi]?  (Its ignore or crowd bit, or an area outside; both ends inclusive.)
__device__ __forceinline__ bool gt_ignored(int flags, double area, double lo, double hi) {
  return (flags & (GT_IGNORE | GT_CROWD)) != 0 || area < lo || area > hi;
}

// ---------------------------------------------------------------------------------------------------- evaluate
// One wave per image: kept rows (at most max_kept of a class) per class, and the objects per (class, area range) that are
// not ignored, added to the header's integer counters.
__global__ void __launch_bounds__(64) coco_count_kernel(DetTable t, int classes, const int32_t* __restrict__ gt_off,
                                                        const int32_t* __restrict__ gt_cls, const double* __restrict__ gt_area,
                                                        const int32_t* __restrict__ gt_flags, int num_gt, CocoParams p, int max_kept,
                                                        CocoHeader* h, int* __restrict__ cnt_det) {
  __shared__ int nd[CMAXC], np[CMAXC * CMAXA];
  const int img = blockIdx.x, lane = threadIdx.x;
  for (int c = lane; c < classes; c += 64) nd[c] = 0;
  for (int q = lane; q < classes * p.A; q += 64) np[q] = 0;
  __syncthreads();
  int g0, ngt, nrow;
  if (image_ok(img, t, num_gt, gt_off, &g0, &ngt, &nrow)) {
    count_class_rows(t, img, nrow, classes, nd);
    for (int k = lane; k < ngt; k += 64) {
      const int c = gt_cls[g0 + k];
      if (c < 0 || c >= classes) continue;
      for (int a = 0; a < p.A; ++a)
        if (!gt_ignored(gt_flags[g0 + k], gt_area[g0 + k], p.area_rng[2 * a], p.area_rng[2 * a + 1])) atomicAdd(&np[c * p.A + a], 1);
    }
  } else if (lane == 0) {
    atomicOr(&h->error, 1);
  }
  __syncthreads();
  for (int c = lane; c < classes; c += 64) cnt_det[(size_t)c * t.num_images + img] = nd[c] < max_kept ? nd[c] : max_kept;
  for (int q = lane; q < classes * p.A; q += 64)
    if (np[q]) atomicAdd(&h->npig[q], np[q]);
}

// The greedy walk for one (image, class), one wave.  The class's rows of the image by descending score (stable in table
// order), the first max_kept of them walked in that order.  Every lane holds two of the image's objects of the class
// (k = lane, lane + 64) with their IoU against the row, and, per area range, which thresholds have taken them.  Per (area
// range, threshold) the walk "non-ignored objects first, `>=` takes, stop at the first ignored one once a match is held" is two
// reductions "largest IoU, highest index wins": over the non-ignored objects not yet taken, and only when that finds none,
// over the ignored ones (a crowd is never used up).  Objects keep their order inside both groups, so the object's own index
// stands for its place in the sorted list.  Writes the rows' scores, ranks and bit words into the class's list.
__global__ void __launch_bounds__(64) coco_match_kernel(DetTable t, const int32_t* __restrict__ gt_off,
                                                        const double* __restrict__ gt_box, const int32_t* __restrict__ gt_cls,
                                                        const double* __restrict__ gt_area, const int32_t* __restrict__ gt_flags,
                                                        int num_gt, CocoParams p, ClassLists L, double* __restrict__ cscore,
                                                        int* __restrict__ crank, int* __restrict__ cword, size_t rows) {
  __shared__ double gbox[CMAXG][4];
  __shared__ double garea[CMAXG];
  __shared__ int gflags[CMAXG];
  __shared__ double dbox[CMAXD][4];
  __shared__ double dscore[CMAXD];
  __shared__ int order[CMAXD];
  __shared__ int taken[CMAXA][CMAXG];   // bit t: taken at threshold t in that area range (read and written by the owning lane only)
  const int c = blockIdx.y, lane = threadIdx.x;
  Segment seg;
  if (!class_segment(t, L, blockIdx.x, c, num_gt, gt_off, dbox, dscore, order, &seg)) return;
  const int keep = seg.rows, nd = seg.nd, g0 = seg.g0;   // the first `keep` (at most the largest detection limit) are walked
  const size_t out = seg.out;
  const int ng = wave_compact(
      seg.ngt, [&](int k) { return gt_cls[g0 + k] == c; },
      [&](int k, int q) {
        const double* g = gt_box + (size_t)(g0 + k) * 4;
        for (int e = 0; e < 4; ++e) gbox[q][e] = g[e];
        garea[q] = gt_area[g0 + k];
        gflags[q] = gt_flags[g0 + k];
      });
  for (int a = 0; a < p.A; ++a) taken[a][lane] = taken[a][lane + 64] = 0;
  __syncthreads();
  for (int r = 0; r < keep && r < nd; ++r) {
    const int j = order[r];
    const double dx = dbox[j][0], dy = dbox[j][1], dw = dbox[j][2], dh = dbox[j][3];
    const double darea = dw * dh;
    double iou[2];
    int flags[2];
    bool have[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int k = lane + 64 * s;
      have[s] = k < ng;
      iou[s] = 0.0;
      flags[s] = 0;
      if (have[s]) {
        const double gx = gbox[k][0], gy = gbox[k][1], gw = gbox[k][2], gh = gbox[k][3];
        flags[s] = gflags[k];
        const double iw = fmin(dx + dw, gx + gw) - fmax(dx, gx), ih = fmin(dy + dh, gy + gh) - fmax(dy, gy);
        if (iw > 0 && ih > 0) {
          const double inter = iw * ih;
          const double uni = (flags[s] & GT_CROWD) ? darea : darea + gw * gh - inter;
          iou[s] = inter / uni;
        }
      }
    }
    for (int a = 0; a < p.A; ++a) {
      const double lo = p.area_rng[2 * a], hi = p.area_rng[2 * a + 1];
      bool ign[2];
      int tk[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int k = lane + 64 * s;
        ign[s] = have[s] && gt_ignored(flags[s], garea[have[s] ? k : 0], lo, hi);
        tk[s] = taken[a][k];
      }
      const bool row_out = darea < lo || darea > hi;
      int word = 0;
      for (int ti = 0; ti < p.T; ++ti) {
        const double thr = fmin(p.iou_thr[ti], 1 - 1e-10);
        int bi = -1, group = 0;
        double best = 0.0;
        for (; group < 2; ++group) {   // 0: the non-ignored objects, 1: the ignored ones
          best = 0.0, bi = -1;
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const bool used = ((tk[s] >> ti) & 1) && !(flags[s] & GT_CROWD);
            if (have[s] && ign[s] == (group == 1) && !used && iou[s] >= thr && (bi < 0 || iou[s] >= best)) {
              best = iou[s];
              bi = lane + 64 * s;
            }
          }
          if (__ballot(bi >= 0) == 0) continue;   // (wave-uniform)
          wave_best_highest_index(best, bi);
          break;
        }
        if (bi >= 0) {
          word |= 1 << ti;
          if (group == 1) word |= 1 << (p.T + ti);
          if ((bi & 63) == lane) tk[bi >> 6] |= 1 << ti;
        } else if (row_out) {
          word |= 1 << (p.T + ti);
        }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) taken[a][lane + 64 * s] = tk[s];
      if (lane == 0) cword[(size_t)a * rows + out + r] = word;
    }
    if (lane == 0) {
      cscore[out + r] = dscore[j];
      crank[out + r] = r;
    }
  }
}

// rank_class_rows (det_table.h; equal scores by image, then rank in the image: a stable sort of the per-image lists put
// one after another): a row's rank and words go to its position in the class's order, in the caller's row arrays.
__global__ void __launch_bounds__(SCAN) coco_rank_kernel(const CocoHeader* h, const double* __restrict__ cscore,
                                                         const int* __restrict__ crank, const int* __restrict__ cword, int A,
                                                         size_t rows, int32_t* __restrict__ row_rank, int32_t* __restrict__ row_word) {
  rank_class_rows(h->ndet, cscore, [&](size_t from, size_t to) {
    row_rank[to] = crank[from];
    for (int a = 0; a < A; ++a) row_word[(size_t)a * rows + to] = cword[(size_t)a * rows + from];
  });
}

// One block per (class, area range x detection limit, threshold): the rows of rank < max_det[m] in class order (the others
// stay in place as holes that count nothing), tp = matched & !ignored, fp = !matched & !ignored, rc = tp / npig,
// pr = tp / (fp + tp + eps) over their running sums, the precision envelope from the end, and for every recall threshold
// the envelope at the first row with rc >= it (np.searchsorted, left; 0 past the end).  The list is walked ONCE from its end,
// SCAN rows at a time: a row's running sums are the class's totals minus what lies behind it, the envelope is a running
// maximum, and the first row with rc >= thr is the row whose tp lifts rc from below thr (or row 0), which writes that
// threshold's entry itself.  npig == 0 leaves the entry at -1.
__global__ void __launch_bounds__(SCAN) coco_accumulate_kernel(const CocoHeader* h, CocoParams p, int classes, size_t rows,
                                                               const int32_t* __restrict__ row_rank,
                                                               const int32_t* __restrict__ row_word, double* __restrict__ precision,
                                                               double* __restrict__ recall) {
  __shared__ int buf[SCAN];
  __shared__ double red[SCAN];
  __shared__ int total_tp, total_fp;
  const int c = blockIdx.x, a = blockIdx.y / p.M, m = blockIdx.y % p.M, ti = blockIdx.z, t = threadIdx.x;
  const int n = h->ndet[c], npig_i = h->npig[c * p.A + a], limit = p.max_det[m];
  const size_t pstride = (size_t)classes * p.A * p.M;                       // between recall thresholds
  const size_t cell = ((size_t)c * p.A + a) * p.M + m;
  double* prec = precision + (size_t)ti * p.R * pstride + cell;
  double* rec = recall + (size_t)ti * pstride + cell;
  if (npig_i == 0) {
    for (int r = t; r < p.R; r += SCAN) prec[r * pstride] = -1.0;
    if (t == 0) *rec = -1.0;
    return;
  }
  const double npig = (double)npig_i;
  const size_t off = class_offset(h->ndet, c);
  const int32_t* word = row_word + (size_t)a * rows + off;
  const int32_t* rank = row_rank + off;
  const int mbit = 1 << ti, ibit = 1 << (p.T + ti);
  if (t == 0) total_tp = total_fp = 0;
  for (int r = t; r < p.R; r += SCAN) prec[r * pstride] = 0.0;
  __syncthreads();
  int ntp = 0, nfp = 0;
  for (int i = t; i < n; i += SCAN) {
    const int w = word[i];
    const bool live = rank[i] < limit && !(w & ibit);
    ntp += live && (w & mbit);
    nfp += live && !(w & mbit);
  }
  if (ntp) atomicAdd(&total_tp, ntp);
  if (nfp) atomicAdd(&total_fp, nfp);
  __syncthreads();
  const int all_tp = total_tp, all_fp = total_fp;
  if (t == 0) *rec = (double)all_tp / npig;        // rc[nd - 1]; 0 when no row is kept
  int behind_tp = 0, behind_fp = 0;                // tp / fp of the chunks already walked (they lie behind this one)
  double carry = 0.0;                              // their envelope (0: "past the end")
  for (int i0 = ((n > 0 ? n - 1 : 0) / SCAN) * SCAN; i0 >= 0 && n > 0; i0 -= SCAN) {
    const int i = i0 + SCAN - 1 - t;               // thread 0 holds the chunk's last row: a prefix over threads is a suffix over rows
    bool kept = false, is_tp = false, is_fp = false;
    if (i < n) {
      const int w = word[i];
      kept = rank[i] < limit;
      is_tp = kept && !(w & ibit) && (w & mbit);
      is_fp = kept && !(w & ibit) && !(w & mbit);
    }
    const int stp = block_scan_incl<Sum>((int)is_tp, buf);   // tp of rows >= i of the chunk
    const int chunk_tp = buf[SCAN - 1];
    const int sfp = block_scan_incl<Sum>((int)is_fp, buf);
    const int chunk_fp = buf[SCAN - 1];
    const int tp = all_tp - behind_tp - (stp - is_tp), fp = all_fp - behind_fp - (sfp - is_fp);   // running sums up to and with row i
    const double dtp = (double)tp;
    const double pr = kept ? dtp / ((double)fp + dtp + 2.220446049250313e-16) : -1.0;
    const double env = Max()(carry, block_scan_incl<Max>(pr, red));   // max of pr over the kept rows >= i
    if (i < n && (is_tp || i == 0)) {
      const double rc = dtp / npig, rc_prev = (double)(tp - is_tp) / npig;
      for (int r = 0; r < p.R; ++r) {
        const double thr = p.rec_thr[r];
        if (rc >= thr && (i == 0 || !(rc_prev >= thr))) prec[r * pstride] = env;
      }
    }
    carry = Max()(carry, red[SCAN - 1]);
    behind_tp += chunk_tp;
    behind_fp += chunk_fp;
  }
}

}  // namespace
}  // namespace sqdet

extern "C" int sqdet_coco_ingest(const float* boxes, const float* probs, const int32_t* cls, const int32_t* count, const double* scales,
                                 int n, int max_out, int classes, double* det_box, double* det_score, int32_t* det_cls,
                                 int32_t* det_count, int32_t* status, int image_offset, int num_images, int cap, sqdet_stream_t stream) {
  using namespace sqdet;
  return ingest_rows<CocoRow>("coco_ingest", boxes, probs, cls, count, scales, n, max_out, classes, SQDET_COCO_MAX_CLASSES,
                              DetTable{det_box, det_score, det_cls, det_count, status, num_images, cap}, image_offset, stream);
}

extern "C" size_t sqdet_coco_eval_workspace_bytes(int num_images, int cap, int classes) {
  using namespace sqdet;
  if (num_images <= 0 || cap <= 0 || classes <= 0) return 0;
  return carve(nullptr, num_images, cap, classes, CMAXT, SQDET_COCO_MAX_RECALL_THRESHOLDS, CMAXA, CMAXM).bytes;
}

extern "C" int sqdet_coco_evaluate(const double* det_box, const double* det_score, const int32_t* det_cls, const int32_t* det_count,
                                   const int32_t* status, int num_images, int cap, int classes, const int32_t* gt_offsets,
                                   const double* gt_box, const int32_t* gt_cls, const double* gt_area, const int32_t* gt_ignore,
                                   int num_gt, const double* iou_thrs, int num_iou, const double* rec_thrs, int num_rec,
                                   const double* area_ranges, int num_area, const int32_t* max_dets, int num_max_dets,
                                   void* workspace, int32_t* row_rank, int32_t* row_word, double* host_precision, double* host_recall,
                                   int32_t* host_npig, int32_t* host_num_det, sqdet_stream_t stream) {
  using namespace sqdet;
  const DetTable t = read_only_table(det_box, det_score, det_cls, det_count, status, num_images, cap);
  if (const int rc = check_scoring_args("coco_evaluate", t, gt_offsets, workspace,
                                        row_rank && row_word && host_precision && host_recall && host_npig && host_num_det && iou_thrs &&
                                            rec_thrs && area_ranges && max_dets,
                                        gt_box && gt_cls && gt_area && gt_ignore, num_gt, classes, SQDET_COCO_MAX_CLASSES))
    return rc;
  SQDET_REQUIRE(num_iou > 0 && num_rec > 0 && num_area > 0 && num_max_dets > 0, "coco_evaluate: an empty threshold list");
  SQDET_UNSUPPORTED(num_iou > CMAXT, "coco_evaluate: %d IoU thresholds (limit %d)", num_iou, CMAXT);
  SQDET_UNSUPPORTED(num_rec > SQDET_COCO_MAX_RECALL_THRESHOLDS, "coco_evaluate: %d recall thresholds (limit %d)", num_rec,
                    SQDET_COCO_MAX_RECALL_THRESHOLDS);
  SQDET_UNSUPPORTED(num_area > CMAXA, "coco_evaluate: %d area ranges (limit %d)", num_area, CMAXA);
  SQDET_UNSUPPORTED(num_max_dets > CMAXM, "coco_evaluate: %d detection limits (limit %d)", num_max_dets, CMAXM);
  for (int m = 0; m < num_max_dets; ++m) {
    SQDET_REQUIRE(max_dets[m] > 0 && (m == 0 || max_dets[m] > max_dets[m - 1]), "coco_evaluate: maxDets must be positive and ascending");
    SQDET_UNSUPPORTED(max_dets[m] > CMAXK, "coco_evaluate: maxDets %d (limit %d)", max_dets[m], CMAXK);
  }
  hipStream_t st = as_stream(stream);
  const int T = num_iou, R = num_rec, A = num_area, M = num_max_dets, max_kept = max_dets[M - 1];
  const CocoWorkspace w = carve(workspace, num_images, cap, classes, T, R, A, M);
  const ClassLists L = {w.cnt_det, w.base, w.h->ndet, num_images};
  const size_t rows = (size_t)num_images * cap;
  const unsigned K = (unsigned)classes, N = (unsigned)num_images;
  CocoLists lists = {};   // (the stream is synchronised before this returns)
  for (int i = 0; i < T; ++i) lists.iou[i] = iou_thrs[i];
  for (int i = 0; i < R; ++i) lists.rec[i] = rec_thrs[i];
  for (int i = 0; i < 2 * A; ++i) lists.area[i] = area_ranges[i];
  for (int i = 0; i < M; ++i) lists.max_det[i] = max_dets[i];
  CocoLists* dl = w.lists;
  SQDET_CHECK_HIP(hipMemcpyAsync(dl, &lists, sizeof(CocoLists), hipMemcpyHostToDevice, st));
  const CocoParams p = {dl->iou, dl->rec, dl->area, dl->max_det, T, R, A, M};
  SQDET_CHECK_HIP(hipMemsetAsync(w.h, 0, sizeof(CocoHeader), st));
  SQDET_CHECK_HIP(hipMemsetAsync(row_rank, 0, rows * sizeof(int32_t), st));
  SQDET_CHECK_HIP(hipMemsetAsync(row_word, 0, (size_t)A * rows * sizeof(int32_t), st));
  hipLaunchKernelGGL(coco_count_kernel, dim3(N), dim3(64), 0, st, t, classes, gt_offsets, gt_cls, gt_area, gt_ignore, num_gt, p, max_kept,
                     w.h, w.cnt_det);
  hipLaunchKernelGGL(class_scan_kernel, dim3(K), dim3(SCAN), 0, st, L);
  hipLaunchKernelGGL(coco_match_kernel, dim3(N, K), dim3(64), 0, st, t, gt_offsets, gt_box, gt_cls, gt_area, gt_ignore, num_gt, p, L,
                     w.cscore, w.crank, w.cword, rows);
  hipLaunchKernelGGL(coco_rank_kernel, dim3((unsigned)((rows + SCAN - 1) / SCAN), K), dim3(SCAN), 0, st, w.h, w.cscore, w.crank, w.cword,
                     A, rows, row_rank, row_word);
  hipLaunchKernelGGL(coco_accumulate_kernel, dim3(K, (unsigned)(A * M), (unsigned)T), dim3(SCAN), 0, st, w.h, p, classes, rows, row_rank,
                     row_word, w.precision, w.recall);
  SQDET_CHECK_HIP(hipGetLastError());
  // header, precision and recall are adjacent: one copy into a staging buffer, so that a failure leaves the host outputs alone
  std::vector<char> stage(w.out_bytes);
  CocoHeader* host = reinterpret_cast<CocoHeader*>(stage.data());
  const size_t head = reinterpret_cast<char*>(w.precision) - reinterpret_cast<char*>(w.h);
  SQDET_CHECK_HIP(hipMemcpyAsync(stage.data() + sizeof(CocoHeader), reinterpret_cast<char*>(w.h) + sizeof(CocoHeader),
                                 w.out_bytes - sizeof(CocoHeader), hipMemcpyDeviceToHost, st));
  if (const int rc = read_back("coco_evaluate", w.h, t, classes, st, host)) return rc;
  const size_t np = (size_t)T * R * classes * A * M, nr = (size_t)T * classes * A * M;
  memcpy(host_precision, stage.data() + head, np * sizeof(double));
  memcpy(host_recall, stage.data() + head + np * sizeof(double), nr * sizeof(double));
  for (int c = 0; c < classes; ++c) {
    host_num_det[c] = host->ndet[c];
    for (int a = 0; a < A; ++a) host_npig[c * A + a] = host->npig[c * A + a];
  }
  return SQDET_OK;
}
