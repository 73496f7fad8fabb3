// The second suppression stage (OURS): greedy NMS, Soft-NMS (Bodla et al. 2017, linear and Gaussian), DIoU-NMS
// (Zheng et al. 2020) and class-agnostic suppression over the <= 64 rows per image that filter_prediction's top-N branch emits
// when it is called with nms_thresh = +inf (it then only selects and orders).  One 256-thread workgroup per image, in place on
// the filter's five outputs:
//
//   1. wave 0: lane r loads row r; the rows' composite keys make_key(prob, anchor index) go to LDS;
//   2. all four waves share the 64 x 64 key comparisons: rank = position in the filter's own descending total order (the
//      rows arrive ordered by class, then rank); the rows are scattered to LDS by rank, lane r is rank r from here on;
//   3. all four waves share the 64 x 64 overlaps (wave w: rows 16w .. 16w+15 against every lane): the hard rules keep one
//      64-bit "i suppresses" mask per row (a ballot), the soft rules the float32 IoU matrix (16 KB of LDS);
//   4. wave 0 resolves the rule: nongreedy = the OR of all masks; greedy = a uniform 64-step walk over an alive mask; soft =
//      at most 64 rounds of a wave-wide argmax by shuffles, then every lane decays its own float64 score from the picked
//      row's matrix line;
//   5. wave 0 writes the survivors ordered by class, then pick order (positions from per-class ballots, as filter_body.h),
//      zeroes the rest and stores the count.
// Every row is read before the first barrier and written after the last: in place is safe.  No atomics; plain vector stores.
// Compiled with -ffp-contract=off: every operator is one IEEE operation, restated in NumPy by tests/nms_options_reference.py.
#include "postproc.h"
#include <cmath>

namespace sqdet {

struct SuppressArgs {
  float* boxes;
  float* probs;
  int32_t* cls;
  int32_t* index;
  int32_t* count;
  int rows, classes;
  int method, overlap, agnostic;
  double nms_thresh, sigma, score_floor;
};

struct SuppressLds {
  unsigned long long key[64];
  unsigned long long sup[64];   // bit j of sup[i]: rank i suppresses rank j (hard rules)
  f32x4 box[64];                // by rank
  float prob[64];
  int cls[64];
  int idx[64];
  int prank[4][64];             // partial ranks, one line per wave
  double score[64];             // soft rules: the final score, by rank
  int ord[64];                  // soft rules: pick order -> rank
  int kept;
  float iou[64][64];            // soft rules
};

// DIoU (Zheng et al. 2020) in float64 on iou_center's float32 corners: iou - d^2 / c^2, d = centre distance, c = diagonal of
// the enclosing box.  0 / 0 (two empty boxes on one point) is NaN: it compares false and never suppresses.
__device__ __forceinline__ double diou_center(float iou, const f32x4& bj, const f32x4& bi) {
  const double dx = (double)bj[0] - (double)bi[0];
  const double dy = (double)bj[1] - (double)bi[1];
  const double ew = (double)fmaxf(bj[0] + 0.5f * bj[2], bi[0] + 0.5f * bi[2]) - (double)fminf(bj[0] - 0.5f * bj[2], bi[0] - 0.5f * bi[2]);
  const double eh = (double)fmaxf(bj[1] + 0.5f * bj[3], bi[1] + 0.5f * bi[3]) - (double)fminf(bj[1] - 0.5f * bj[3], bi[1] - 0.5f * bi[3]);
  return (double)iou - (dx * dx + dy * dy) / (ew * ew + eh * eh);
}

__global__ __launch_bounds__(256) void suppress_kernel(SuppressArgs a) {
  __shared__ SuppressLds s;
  const int img = blockIdx.x;
  const int tid = threadIdx.x, r = tid & 63, wv = tid >> 6;
  const int cnt = a.count[img];
  if (cnt < 0 || cnt > a.rows) return;   // the filter's overflow report (or garbage): the image passes through (uniform)
  float* ob = a.boxes + (size_t)img * a.rows * 4;
  float* op = a.probs + (size_t)img * a.rows;
  int32_t* oc = a.cls + (size_t)img * a.rows;
  int32_t* oi = a.index + (size_t)img * a.rows;
  const bool soft = a.method >= SQDET_NMS_SOFT_LINEAR;

  // ---- 1. lane r of wave 0 loads row r
  f32x4 b = {0.f, 0.f, 0.f, 0.f};
  float p = 0.f;
  int c = -1, idx = -1;
  if (wv == 0) {
    if (r < cnt) {
      b = *reinterpret_cast<const f32x4*>(ob + (size_t)r * 4);
      p = op[r];
      c = oc[r];
      idx = oi[r];
    }
    s.key[r] = r < cnt ? make_key(p, idx) : 0ull;
  }
  __syncthreads();

  // ---- 2. rank of row r among the cnt rows, descending key (equal keys -- never from the filter, whose anchor indices are
  //         distinct -- : the lower row first, so the ranks are always a permutation of [0, cnt))
  {
    const unsigned long long mine = s.key[r];
    int part = 0;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = wv * 16 + u;
      const unsigned long long o = s.key[i];
      part += (i < cnt && (o > mine || (o == mine && i < r))) ? 1 : 0;
    }
    s.prank[wv][r] = part;
  }
  __syncthreads();
  if (wv == 0) {
    const int rank = r < cnt ? s.prank[0][r] + s.prank[1][r] + s.prank[2][r] + s.prank[3][r] : r;
    s.box[rank] = b;
    s.prob[rank] = p;
    s.cls[rank] = c;
    s.idx[rank] = idx;
  }
  __syncthreads();

  // ---- 3. lane r is rank r.  A row takes part iff its class is a class (the filter's own keep test).
  const f32x4 br = s.box[r];
  const int cr = s.cls[r];
  const bool vr = r < cnt && cr >= 0 && cr < a.classes;
#pragma unroll 4
  for (int u = 0; u < 16; ++u) {
    const int i = wv * 16 + u;
    const f32x4 bi = s.box[i];
    const int ci = s.cls[i];
    const bool vi = i < cnt && ci >= 0 && ci < a.classes;
    const float ov = iou_center(br, bi);   // (lower-ranked, higher-ranked) as the filter calls it; symmetric bit for bit
    if (soft) {
      s.iou[i][r] = ov;
    } else {
      const double o = a.overlap == SQDET_NMS_OVERLAP_DIOU ? diou_center(ov, br, bi) : (double)ov;
      const bool sup = vi && vr && i < r && (a.agnostic || ci == cr) && o > a.nms_thresh;
      const unsigned long long m = __ballot(sup);
      if (r == 0) s.sup[i] = m;
    }
  }
  __syncthreads();

  // ---- 4. wave 0 resolves the rule
  bool keep = false;
  if (wv == 0) {
    if (!soft) {
      const unsigned long long valid = __ballot(vr);
      unsigned long long alive = valid;
      if (a.method == SQDET_NMS_NONGREEDY) {
        unsigned long long dropped = 0ull;
        for (int i = 0; i < 64; ++i) dropped |= s.sup[i];
        alive = valid & ~dropped;
      } else {
        for (int i = 0; i < 64; ++i)   // uniform: every lane walks the same mask
          if ((alive >> i) & 1ull) alive &= ~s.sup[i];
      }
      keep = (alive >> r) & 1ull;
    } else {
      double sc = (double)s.prob[r];
      bool rem = vr;
      int myord = -1, kept = 0;
      for (int round = 0; round < 64; ++round) {
        // argmax of the remaining scores, a tie to the higher rank (= lower lane); a lane that is out carries lane 64
        double bs = rem ? sc : 0.0;
        int bj = rem ? r : 64;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double os = __shfl_xor(bs, off);
          const int oj = __shfl_xor(bj, off);
          if (oj < 64 && (bj >= 64 || os > bs || (os == bs && oj < bj))) { bs = os; bj = oj; }
        }
        bs = __shfl(bs, 0);   // (one answer for the wave even where NaN scores break the order)
        bj = __shfl(bj, 0);
        if (bj >= 64 || bs < a.score_floor) break;
        if (r == bj) { rem = false; myord = kept; }
        ++kept;
        if (rem && (a.agnostic || cr == s.cls[bj])) {
          const double o = (double)s.iou[bj][r];
          if (a.method == SQDET_NMS_SOFT_LINEAR) {
            if (o > a.nms_thresh) sc = sc * (1.0 - o);
          } else {
            sc = sc * exp(-(o * o) / a.sigma);
          }
        }
      }
      if (myord >= 0) { s.ord[myord] = r; s.score[r] = sc; }
      if (r == 0) s.kept = kept;
    }
  }
  __syncthreads();

  // ---- 5. wave 0 emits: lane k is the k-th row in pick order (hard rules: rank order, the dropped ones masked out)
  if (wv == 0) {
    int src = r;
    float pj = 0.f;
    if (soft) {
      keep = r < s.kept;
      src = keep ? s.ord[r] : 0;
      pj = keep ? (float)s.score[src] : 0.f;
    } else {
      pj = s.prob[r];
    }
    const int cj = keep ? s.cls[src] : -1;
    const unsigned long long km = __ballot(keep);
    const int kept = __popcll(km);
    int pos = 0;
    {
      const unsigned long long below = r == 0 ? 0ull : (~0ull >> (64 - r));
      for (int cc = 0; cc < a.classes; ++cc) {   // uniform trip count
        const unsigned long long mc = __ballot(cj == cc) & km;
        pos += cc < cj ? __popcll(mc) : (cc == cj ? __popcll(mc & below) : 0);
      }
    }
    if (keep) {
      *reinterpret_cast<f32x4*>(ob + (size_t)pos * 4) = s.box[src];
      op[pos] = pj;
      oc[pos] = cj;
      oi[pos] = s.idx[src];
    }
    for (int o = kept + r; o < a.rows; o += 64) {
      *reinterpret_cast<f32x4*>(ob + (size_t)o * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
      op[o] = 0.f;
      oc[o] = -1;
      oi[o] = -1;
    }
    if (r == 0) a.count[img] = kept;
  }
}

}  // namespace sqdet

using namespace sqdet;

extern "C" int sqdet_suppress_rows(float* boxes, float* probs, int32_t* cls, int32_t* index, int32_t* count, int n, int rows,
                                   int classes, const sqdet_nms_options_t* opt, sqdet_stream_t stream) {
  SQDET_REQUIRE(boxes && probs && cls && index && count && opt, "suppress_rows: null pointer");
  SQDET_REQUIRE(n > 0 && classes > 0, "suppress_rows: bad dims");
  SQDET_REQUIRE(rows >= 1 && rows <= 64, "suppress_rows: rows %d outside 1..64 (TOP_N_DETECTION <= 64)", rows);
  SQDET_REQUIRE(opt->method >= SQDET_NMS_NONGREEDY && opt->method <= SQDET_NMS_SOFT_GAUSSIAN, "suppress_rows: unknown method %d",
                opt->method);
  SQDET_REQUIRE(opt->overlap == SQDET_NMS_OVERLAP_IOU || opt->overlap == SQDET_NMS_OVERLAP_DIOU, "suppress_rows: unknown overlap %d",
                opt->overlap);
  SQDET_REQUIRE(!(opt->overlap == SQDET_NMS_OVERLAP_DIOU && opt->method >= SQDET_NMS_SOFT_LINEAR),
                "suppress_rows: the diou overlap goes with the hard methods only (nongreedy, greedy)");
  SQDET_REQUIRE(opt->sigma > 0.0, "suppress_rows: sigma must be > 0");
  SQDET_REQUIRE(std::isfinite(opt->score_floor), "suppress_rows: score_floor must be finite");
  SuppressArgs a;
  a.boxes = boxes; a.probs = probs; a.cls = cls; a.index = index; a.count = count;
  a.rows = rows; a.classes = classes;
  a.method = opt->method; a.overlap = opt->overlap; a.agnostic = opt->class_agnostic ? 1 : 0;
  a.nms_thresh = opt->nms_thresh; a.sigma = opt->sigma; a.score_floor = opt->score_floor;
  hipLaunchKernelGGL(suppress_kernel, dim3(n), dim3(256), 0, as_stream(stream), a);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}
