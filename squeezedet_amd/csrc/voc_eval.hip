// Pascal VOC detection scoring on the GPU: the reference's VOC path after the detector (src/dataset/pascal_voc.py:81-137,
// src/dataset/voc_eval.py) without text files, for every class at once.
//
//   ingest    filter_prediction rows -> the device detection table (det_table.h, VocRow), each value exactly the double
//             float() reads back from the per-class files pascal_voc.evaluate_detections writes (coordinates + 1 in
//             float32, rounded as '{:.1f}', scores as '{:.3f}');
//   evaluate  voc_eval for all classes: count (rows and non-difficult objects per image and class), scan (where each
//             (image, class) segment starts in its class's list), match (one wave per (image, class): the greedy walk of
//             voc_eval.py:161-195), rank (each row's position in its class's order), prefix (cumulative tp / fp) and
//             ap (recall, precision, the 11-point AP and the area under the precision envelope).
//
// Everything is double precision with -ffp-contract=off (build.py): overlaps, recall, precision and the 11-point sum are
// bitwise those of NumPy.  Counts are integers and every sum has a fixed order, so results do not depend on scheduling.
#include <float.h>

#include "det_table.h"   // the table, its ingest ('{:.1f}' / '{:.3f}' as the detection files carry them) and the shared helpers

namespace sqdet {
namespace {

constexpr int VMAXD = DT_MAX_ROWS;                // detection rows per image
constexpr int VMAXG = DT_MAX_GT;                  // ground-truth rows per image
constexpr int VMAXC = SQDET_VOC_MAX_CLASSES;
constexpr int SCAN = DT_RANK;                     // threads of the scan / rank / ap blocks: a class longer than this loops
constexpr int NT07 = 11;                          // thresholds of the 11-point metric
enum { FLAG_NONE = 0, FLAG_TP = 1, FLAG_FP = 2 };

struct VocHeader {
  int error;  // an image over the row limits was seen (it is scored as empty; the call fails)
  int pad;
  int npos[VMAXC];  // non-difficult objects
  int ndet[VMAXC];  // rows
  double ap07[VMAXC];
  double ap_area[VMAXC];
};

// The workspace of sqdet_voc_evaluate; the per-row arrays ([T]) hold the class lists of det_table.h, rows in table order.
struct VocWorkspace {
  VocHeader* h;
  double* cscore;  // [T] score, class lists
  double* mpre;    // [T] suffix maximum of precision, class order
  int* cnt_det;    // [C, N] rows of the class in the image
  int* base;       // [C, N] exclusive prefix of cnt_det over the images
  int* cflag;      // [T] FLAG_*, class lists
  int* stp;        // [T] tp flags in class order, then their running sum
  int* sfp;        // [T] fp likewise
  size_t bytes;
};

VocWorkspace carve(void* p, int num_images, int cap, int classes) {
  const size_t T = (size_t)num_images * cap, CN = (size_t)classes * num_images;
  Carver k{reinterpret_cast<char*>(p)};
  VocWorkspace w;
  w.h = k.take<VocHeader>(1);
  w.cscore = k.take<double>(T, 256);
  w.mpre = k.take<double>(T);
  w.cnt_det = k.take<int>(CN);
  w.base = k.take<int>(CN);
  w.cflag = k.take<int>(T);
  w.stp = k.take<int>(T);
  w.sfp = k.take<int>(T);   // (adjacent to stp: one memset clears both)
  w.bytes = k.o;
  return w;
}

// ---------------------------------------------------------------------------------------------------- evaluate
// One wave per image: rows of every class, and its non-difficult objects (voc_eval.py:127-132) added to the header's
// integer counters.
__global__ void __launch_bounds__(64) voc_count_kernel(DetTable t, int classes, const int32_t* __restrict__ gt_off,
                                                       const int32_t* __restrict__ gt_cls, const int32_t* __restrict__ gt_difficult,
                                                       int num_gt, VocHeader* h, int* __restrict__ cnt_det) {
  __shared__ int nd[VMAXC], np[VMAXC];
  const int img = blockIdx.x, lane = threadIdx.x;
  for (int c = lane; c < classes; c += 64) nd[c] = np[c] = 0;
  __syncthreads();
  int g0, ngt, nrow;
  if (image_ok(img, t, num_gt, gt_off, &g0, &ngt, &nrow)) {
    count_class_rows(t, img, nrow, classes, nd);
    for (int k = lane; k < ngt; k += 64) {
      const int c = gt_cls[g0 + k];
      if (c >= 0 && c < classes && !gt_difficult[g0 + k]) atomicAdd(&np[c], 1);
    }
  } else if (lane == 0) {
    atomicOr(&h->error, 1);
  }
  __syncthreads();
  for (int c = lane; c < classes; c += 64) {
    cnt_det[(size_t)c * t.num_images + img] = nd[c];
    if (np[c]) atomicAdd(&h->npos[c], np[c]);
  }
}

// voc_eval.py:161-195 for one (image, class), one wave: the class's rows of the image by descending score (stable in table
// order), each against the image's objects of the class -- lanes compute the overlaps, the wave takes the maximum with the
// first index winning (np.argmax) -- then the tp / fp / neither decision.  Writes the rows' scores and flags into the
// class's list.
__global__ void __launch_bounds__(64) voc_match_kernel(DetTable t, const int32_t* __restrict__ gt_off,
                                                       const double* __restrict__ gt_box, const int32_t* __restrict__ gt_cls,
                                                       const int32_t* __restrict__ gt_difficult, int num_gt, ClassLists L,
                                                       double* __restrict__ cscore, int* __restrict__ cflag) {
  __shared__ double gbox[VMAXG][4];
  __shared__ int gdiff[VMAXG];
  __shared__ int gtaken[VMAXG];
  __shared__ double dbox[VMAXD][4];
  __shared__ double dscore[VMAXD];
  __shared__ int order[VMAXD];
  __shared__ int dflag[VMAXD];
  const int c = blockIdx.y, lane = threadIdx.x;
  Segment s;
  if (!class_segment(t, L, blockIdx.x, c, num_gt, gt_off, dbox, dscore, order, &s)) return;
  const int nd = s.nd, g0 = s.g0;
  // the image's objects of the class, order kept
  const int ng = wave_compact(
      s.ngt, [&](int k) { return gt_cls[g0 + k] == c; },
      [&](int k, int p) {
        const double* g = gt_box + (size_t)(g0 + k) * 4;
        for (int q = 0; q < 4; ++q) gbox[p][q] = g[q];
        gdiff[p] = gt_difficult[g0 + k] != 0;
        gtaken[p] = 0;
      });
  __syncthreads();
  for (int r = 0; r < nd; ++r) {
    const int j = order[r];
    const double b0 = dbox[j][0], b1 = dbox[j][1], b2 = dbox[j][2], b3 = dbox[j][3];
    double best = 0;
    int bi = -1;
    for (int k = lane; k < ng; k += 64) {
      const double ixmin = fmax(gbox[k][0], b0), iymin = fmax(gbox[k][1], b1);
      const double ixmax = fmin(gbox[k][2], b2), iymax = fmin(gbox[k][3], b3);
      const double iw = fmax(ixmax - ixmin + 1., 0.), ih = fmax(iymax - iymin + 1., 0.);
      const double inters = iw * ih;
      const double uni = ((b2 - b0 + 1.) * (b3 - b1 + 1.) + (gbox[k][2] - gbox[k][0] + 1.) * (gbox[k][3] - gbox[k][1] + 1.) - inters);
      const double ov = inters / uni;
      if (bi < 0 || ov > best) {
        best = ov;
        bi = k;
      }
    }
    wave_best_lowest_index(best, bi);  // greatest overlap, lowest index on ties
    int f = FLAG_FP;  // no object of the class in the image (ovmax = -inf), or ovmax <= ovthresh
    if (bi >= 0 && best > 0.5) {
      if (gdiff[bi]) f = FLAG_NONE;
      else if (!gtaken[bi]) f = FLAG_TP;
    }
    __syncthreads();
    if (lane == 0) {
      dflag[j] = f;
      if (f == FLAG_TP) gtaken[bi] = 1;
    }
    __syncthreads();
  }
  for (int j = lane; j < nd; j += 64) {
    cscore[s.out + j] = dscore[j];
    cflag[s.out + j] = dflag[j];
  }
}

// rank_class_rows (det_table.h; equal scores by image, then row): a row's flags go to its position in the class's order.
__global__ void __launch_bounds__(SCAN) voc_rank_kernel(const VocHeader* h, const double* __restrict__ cscore,
                                                        const int* __restrict__ cflag, int* __restrict__ stp, int* __restrict__ sfp) {
  rank_class_rows(h->ndet, cscore, [&](size_t from, size_t to) {
    const int f = cflag[from];
    stp[to] = f == FLAG_TP;
    sfp[to] = f == FLAG_FP;
  });
}

// np.cumsum of tp and fp (voc_eval.py:198-199), one block per class, SCAN rows at a time with the running total carried.
__global__ void __launch_bounds__(SCAN) voc_prefix_kernel(const VocHeader* h, int* __restrict__ stp, int* __restrict__ sfp) {
  __shared__ int buf[SCAN];
  const int c = blockIdx.x, n = h->ndet[c], t = threadIdx.x;
  const size_t off = class_offset(h->ndet, c);
  int ctp = 0, cfp = 0;
  for (int i0 = 0; i0 < n; i0 += SCAN) {
    const int i = i0 + t;
    const int a = block_scan_incl<Sum>(i < n ? stp[off + i] : 0, buf);
    const int ta = buf[SCAN - 1];
    const int b = block_scan_incl<Sum>(i < n ? sfp[off + i] : 0, buf);
    const int tb = buf[SCAN - 1];
    if (i < n) {
      stp[off + i] = ctp + a;
      sfp[off + i] = cfp + b;
    }
    ctp += ta;
    cfp += tb;
  }
}

__device__ __forceinline__ void rec_prec(int tp, int fp, double npos, double* rec, double* prec) {
  const double dtp = (double)tp, s = dtp + (double)fp;
  *rec = dtp / npos;                          // (0 / 0 = NaN for a class without objects, as NumPy's)
  *prec = dtp / (s < DBL_EPSILON ? DBL_EPSILON : s);
}

// voc_eval.py:200-204 and voc_ap (:33-64), one block per class.
__global__ void __launch_bounds__(SCAN) voc_ap_kernel(VocHeader* h, const int* __restrict__ stp, const int* __restrict__ sfp,
                                                      double* __restrict__ mpre, int curve_cls, double* __restrict__ curve_rec,
                                                      double* __restrict__ curve_prec) {
  __shared__ double red[SCAN];
  __shared__ double wave_max[SCAN / 64][NT07];
  const int c = blockIdx.x, n = h->ndet[c], t = threadIdx.x;
  if (n == 0) {  // no detections: voc_eval returns 0 (:147-148)
    if (t == 0) h->ap07[c] = h->ap_area[c] = 0.0;
    return;
  }
  const size_t off = class_offset(h->ndet, c);
  const double npos = (double)h->npos[c];
  // ---- the 11-point metric: p_q = max(prec[rec >= q * 0.1]), 0 when there is none (-1 marks "none": prec >= 0)
  double m[NT07];
#pragma unroll
  for (int q = 0; q < NT07; ++q) m[q] = -1.0;
  for (int i = t; i < n; i += SCAN) {
    double rec, prec;
    rec_prec(stp[off + i], sfp[off + i], npos, &rec, &prec);
    if (c == curve_cls) {
      curve_rec[i] = rec;
      curve_prec[i] = prec;
    }
#pragma unroll
    for (int q = 0; q < NT07; ++q)
      if (rec >= (double)q * 0.1 && prec > m[q]) m[q] = prec;   // np.arange(0., 1.1, 0.1)[q] = q * 0.1
  }
#pragma unroll
  for (int q = 0; q < NT07; ++q) {
    double v = m[q];
    for (int o = 32; o > 0; o >>= 1) {
      const double x = __shfl_xor(v, o);
      v = x > v ? x : v;
    }
    if ((t & 63) == 0) wave_max[t >> 6][q] = v;
  }
  __syncthreads();
  if (t == 0) {
    double ap = 0.;
    for (int q = 0; q < NT07; ++q) {
      double p = wave_max[0][q];
      for (int w = 1; w < SCAN / 64; ++w) p = wave_max[w][q] > p ? wave_max[w][q] : p;
      if (p < 0) p = 0.;
      ap = ap + p / 11.;
    }
    h->ap07[c] = ap;
  }
  // ---- the precision envelope (:55-56): mpre[i] = max(prec[i:]) (the trailing sentinel is 0 <= prec), SCAN rows at a time
  // from the end with the running maximum carried
  double carry = 0.;
  for (int i0 = ((n - 1) / SCAN) * SCAN; i0 >= 0; i0 -= SCAN) {
    const int i = i0 + SCAN - 1 - t;   // thread 0 holds the chunk's last row: a prefix over threads is a suffix over rows
    double rec, prec = 0.;
    if (i < n) rec_prec(stp[off + i], sfp[off + i], npos, &rec, &prec);
    const double env = Max()(carry, block_scan_incl<Max>(prec, red));
    if (i < n) mpre[off + i] = env;
    carry = Max()(carry, red[SCAN - 1]);
  }
  __syncthreads();
  // ---- sum (mrec[i + 1] - mrec[i]) * mpre[i + 1] where recall changes (:60-63): a strided partial per thread, then a
  // fixed tree (NumPy sums pairwise: the area form may differ from it in the last bits, see sqdet.h)
  double s = 0.;
  for (int i = t; i < n; i += SCAN) {
    double rec, prev = 0., prec;
    rec_prec(stp[off + i], sfp[off + i], npos, &rec, &prec);
    if (i > 0) rec_prec(stp[off + i - 1], sfp[off + i - 1], npos, &prev, &prec);
    if (rec != prev) s += (rec - prev) * mpre[off + i];
    if (i == n - 1 && 1. != rec) s += (1. - rec) * 0.;   // the trailing sentinel's term: 0, or NaN with a NaN recall
  }
  red[t] = s;
  __syncthreads();
  for (int o = SCAN / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) h->ap_area[c] = red[0];
}

}  // namespace
}  // namespace sqdet

extern "C" int sqdet_voc_ingest(const float* boxes, const float* probs, const int32_t* cls, const int32_t* count, const double* scales,
                                int n, int max_out, int classes, double* det_box, double* det_score, int32_t* det_cls,
                                int32_t* det_count, int32_t* status, int image_offset, int num_images, int cap, sqdet_stream_t stream) {
  using namespace sqdet;
  return ingest_rows<VocRow>("voc_ingest", boxes, probs, cls, count, scales, n, max_out, classes, SQDET_VOC_MAX_CLASSES,
                             DetTable{det_box, det_score, det_cls, det_count, status, num_images, cap}, image_offset, stream);
}

extern "C" size_t sqdet_voc_eval_workspace_bytes(int num_images, int cap, int classes) {
  if (num_images <= 0 || cap <= 0 || classes <= 0) return 0;
  return sqdet::carve(nullptr, num_images, cap, classes).bytes;
}

extern "C" int sqdet_voc_evaluate(const double* det_box, const double* det_score, const int32_t* det_cls, const int32_t* det_count,
                                  const int32_t* status, int num_images, int cap, int classes, const int32_t* gt_offsets,
                                  const double* gt_box, const int32_t* gt_cls, const int32_t* gt_difficult, int num_gt, void* workspace,
                                  double* host_ap07, double* host_ap_area, int32_t* host_npos, int32_t* host_num_det, int curve_cls,
                                  double* curve_rec, double* curve_prec, sqdet_stream_t stream) {
  using namespace sqdet;
  const DetTable t = read_only_table(det_box, det_score, det_cls, det_count, status, num_images, cap);
  if (const int rc = check_scoring_args("voc_evaluate", t, gt_offsets, workspace, host_ap07 && host_ap_area && host_npos && host_num_det,
                                        gt_box && gt_cls && gt_difficult, num_gt, classes, SQDET_VOC_MAX_CLASSES))
    return rc;
  SQDET_REQUIRE(curve_cls < classes && (curve_cls < 0 || (curve_rec && curve_prec)), "voc_evaluate: bad curve class or null curve buffer");
  hipStream_t st = as_stream(stream);
  const VocWorkspace w = carve(workspace, num_images, cap, classes);
  const ClassLists L = {w.cnt_det, w.base, w.h->ndet, num_images};
  const size_t T = (size_t)num_images * cap;
  const unsigned C = (unsigned)classes, N = (unsigned)num_images;
  SQDET_CHECK_HIP(hipMemsetAsync(w.h, 0, sizeof(VocHeader), st));
  SQDET_CHECK_HIP(hipMemsetAsync(w.stp, 0, 2 * T * sizeof(int), st));   // stp and sfp are adjacent
  hipLaunchKernelGGL(voc_count_kernel, dim3(N), dim3(64), 0, st, t, classes, gt_offsets, gt_cls, gt_difficult, num_gt, w.h, w.cnt_det);
  hipLaunchKernelGGL(class_scan_kernel, dim3(C), dim3(SCAN), 0, st, L);
  hipLaunchKernelGGL(voc_match_kernel, dim3(N, C), dim3(64), 0, st, t, gt_offsets, gt_box, gt_cls, gt_difficult, num_gt, L, w.cscore,
                     w.cflag);
  hipLaunchKernelGGL(voc_rank_kernel, dim3((unsigned)((T + SCAN - 1) / SCAN), C), dim3(SCAN), 0, st, w.h, w.cscore, w.cflag, w.stp, w.sfp);
  hipLaunchKernelGGL(voc_prefix_kernel, dim3(C), dim3(SCAN), 0, st, w.h, w.stp, w.sfp);
  hipLaunchKernelGGL(voc_ap_kernel, dim3(C), dim3(SCAN), 0, st, w.h, w.stp, w.sfp, w.mpre, curve_cls, curve_rec, curve_prec);
  SQDET_CHECK_HIP(hipGetLastError());
  VocHeader host;
  if (const int rc = read_back("voc_evaluate", w.h, t, classes, st, &host)) return rc;
  for (int c = 0; c < classes; ++c) {
    host_ap07[c] = host.ap07[c];
    host_ap_area[c] = host.ap_area[c];
    host_npos[c] = host.npos[c];
    host_num_det[c] = host.ndet[c];
  }
  return SQDET_OK;
}
