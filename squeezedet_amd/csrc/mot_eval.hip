// Tracking evaluation on the device (sqdet_mot_update, sqdet_mot_evaluate; include/sqdet.h, "tracking evaluation"): the CLEAR-MOT
// counts and IDF1 of the tracker's outputs against labelled objects, computed where the tracker leaves its identities.  The
// reference has nothing of the kind; the definition is the header's, restated sequentially in tests/mot_reference.py.
//
// sqdet_mot_update: one WAVE per stream, walking its F frames in order.  A frame has at most 64 objects and 64 hypotheses, so
// lane o IS object row o for everything an object does (validity, its identity, continuity, its table entries, its row of
// `overlap`) and lane h IS hypothesis row h for what a hypothesis does.  The (object, hypothesis) IoUs are dealt to the 64 lanes in
// turn as track.hip deals its pairs.  A class's five counters and its iou_sum live in the registers of lane c (and c + 64) for the
// whole call: every lane walks the frame's objects in row order and adds what belongs to its class, so iou_sum is summed in the
// order of the definition without a lane ever writing another's word.  The stream's identity tables sit in LDS; a row's identity
// is found by a lane-parallel compare, 64 entries a step.
//
// assign<>() below is the header's assign(): columns on the threads (one per lane in the update kernel, four per thread of the
// 256 in the evaluation kernel), a (value, column) arg-min per round.  Both kernels call the one function, so the per-frame
// matching and IDF1's global matching follow the same text.
//
// Only plain vector loads and stores; no atomics; nothing is allocated.  -ffp-contract=off (build.py): the IoU and the cost
// floor((1 - IoU) * 2^20) are one IEEE operation per operator, compared bit for bit.
#include <vector>
#include <string.h>
#include "stream_wave.h"

namespace sqdet {
namespace {

constexpr int CAP = SQDET_MOT_CAP;
constexpr int MAXO = SQDET_MOT_MAX_OBJECTS, MAXH = SQDET_MOT_MAX_HYPOTHESES;
constexpr int KOUT = SQDET_MOT_COUNTERS;
constexpr int MSTRIDE = CAP + 1;
constexpr long long BIG = 1ll << 32, INF = 1ll << 62;
constexpr int EV_THREADS = 256, EV_COLS = MAXH / EV_THREADS;
static_assert(CAP == 64, "one row per lane of a wave");
static_assert(MAXO % CAP == 0 && MAXH % CAP == 0 && MAXO <= MAXH && EV_COLS * EV_THREADS == MAXH && MAXO <= EV_THREADS, "table sizes");
static_assert(SQDET_MOT_MAX_CLASSES == 2 * CAP, "two classes per lane");

struct MotArgs {
  sqdet_mot_tables_t t;
  const float* boxes;
  const int32_t* cls;
  const int32_t* counts;
  const int32_t* ids;
  const int32_t* states;
  const double* gt_box;
  const int32_t* gt_id;
  const int32_t* gt_cls;
  const int32_t* gt_flags;
  const int32_t* gt_count;
  int S, F, rows, G, classes;
  double iou_thresh;
};

__device__ __forceinline__ long long shfl_xor64(long long v, int m) {
  const int lo = __shfl_xor((int)(unsigned long long)v, m), hi = __shfl_xor((int)((unsigned long long)v >> 32), m);
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// assign() of the header on an R x C matrix, R <= C <= THREADS * COLS: column j belongs to thread j % THREADS.  On return
// s_p[j] is the row of column j, -1 for a free one.  s_u: R words; s_p, s_way: C words; s_wv, s_wj: one word per wave.  Every
// thread of the workgroup calls it with the same R, C and cost.
template <int THREADS, int COLS, class Cost>
__device__ __forceinline__ void assign(int R, int C, Cost cost, long long* s_u, int* s_p, int* s_way, long long* s_wv, int* s_wj, int tid) {
  constexpr int WAVES = THREADS / 64;
  long long v[COLS], minv[COLS];
  int way[COLS];
  bool used[COLS];
#pragma unroll
  for (int k = 0; k < COLS; ++k) {
    v[k] = 0;
    if (tid + THREADS * k < C) s_p[tid + THREADS * k] = -1;
  }
  for (int i = tid; i < R; i += THREADS) s_u[i] = 0;
  __syncthreads();
  for (int i = 0; i < R; ++i) {
#pragma unroll
    for (int k = 0; k < COLS; ++k) { minv[k] = INF; way[k] = -1; used[k] = false; }
    int i0 = i, j0 = -1;
    while (true) {
      const long long u0 = s_u[i0];
      long long bv = INF;
      int bj = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < COLS; ++k) {
        const int j = tid + THREADS * k;
        if (j < C) {
          if (j == j0) used[k] = true;
          if (!used[k]) {
            const long long cur = cost(i0, j) - u0 - v[k];
            if (cur < minv[k]) { minv[k] = cur; way[k] = j0; }
            if (minv[k] < bv) { bv = minv[k]; bj = j; }          // (j ascends with k: the lowest column among equals)
          }
        }
      }
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        const long long ov = shfl_xor64(bv, m);
        const int oj = __shfl_xor(bj, m);
        if (ov < bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
      }
      if (WAVES > 1) {
        if ((tid & 63) == 0) { s_wv[tid >> 6] = bv; s_wj[tid >> 6] = bj; }
        __syncthreads();
        bv = s_wv[0]; bj = s_wj[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
          const long long ov = s_wv[w];
          const int oj = s_wj[w];
          if (ov < bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
        }
      } else {
        __syncthreads();                // every lane has read u0 before a potential moves
      }
      const long long delta = bv;
#pragma unroll
      for (int k = 0; k < COLS; ++k) {
        const int j = tid + THREADS * k;
        if (j < C) {
          if (used[k]) { s_u[s_p[j]] += delta; v[k] -= delta; }   // (scanned columns hold distinct rows, none of them row i)
          else minv[k] -= delta;
        }
      }
      if (tid == 0) s_u[i] += delta;
      __syncthreads();
      j0 = bj;
      const int pj = s_p[j0];
      if (pj < 0) break;
      i0 = pj;
    }
#pragma unroll
    for (int k = 0; k < COLS; ++k)
      if (tid + THREADS * k < C) s_way[tid + THREADS * k] = way[k];
    __syncthreads();
    if (tid == 0) {
      for (int j = j0; j >= 0;) {
        const int w = s_way[j];
        s_p[j] = w >= 0 ? s_p[w] : i;
        j = w;
      }
    }
    __syncthreads();
  }
}

// The value of `v` in lane `r` (uniform r): a register read, no LDS round trip.
__device__ __forceinline__ int lane_value(int v, int r) { return __builtin_amdgcn_readlane(v, r); }
__device__ __forceinline__ double lane_value(double v, int r) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, r), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), r);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// The dense indices of the rows of `need` (uniform; lane r holds row r's identity in `id`, > 0) among the first n entries of the
// LDS table: lane r's result, -1 if its identity has none.  The lanes hold 64 table entries at a time and the rows are passed
// over them one register read each.
__device__ __forceinline__ int find_ids(const int* table, int n, int id, uint64_t need, int lane) {
  int idx = -1;
  for (int k = 0; k < n && need; k += CAP) {
    const int te = k + lane < n ? table[k + lane] : 0;
    for (uint64_t m = need; m; m &= m - 1) {
      const int r = __builtin_ctzll(m);
      const uint64_t hit = __ballot(te == lane_value(id, r));
      if (hit) {
        if (lane == r) idx = k + __builtin_ctzll(hit);
        need &= ~(1ull << r);
      }
    }
  }
  return idx;
}

__global__ void __launch_bounds__(CAP) mot_update_kernel(const MotArgs a) {
  __shared__ double s_iou[CAP * MSTRIDE];
  __shared__ int s_q[CAP * MSTRIDE];                                   // the pair's integer cost, -1: not allowed
  __shared__ double s_obox[CAP][4], s_hbox[CAP][4];
  __shared__ int s_objid[MAXO], s_hypid[MAXH];
  __shared__ int s_oid[CAP], s_hid[CAP], s_ocls[CAP], s_hcls[CAP], s_olist[CAP], s_hlist[CAP], s_taken[CAP], s_omatch[CAP], s_hdrop[CAP], s_hti[CAP], s_rowobj[CAP], s_colhyp[CAP], s_p[CAP], s_way[CAP];
  __shared__ long long s_u[CAP], s_wv[1];
  __shared__ int s_wj[1];
  const int lane = threadIdx.x, rows = a.rows, G = a.G, classes = a.classes;

  for (int s = blockIdx.x; s < a.S; s += gridDim.x) {
    int n_obj = a.t.n_obj[s], n_hyp = a.t.n_hyp[s], status = a.t.status[s];
    n_obj = clamp_count(n_obj, MAXO);                                 // (a loaded table is the caller's: stay inside it)
    n_hyp = clamp_count(n_hyp, MAXH);
    __syncthreads();                    // the previous stream's tables are no longer read
    for (int e = lane; e < n_obj; e += CAP) s_objid[e] = a.t.obj_id[(size_t)s * MAXO + e];
    for (int e = lane; e < n_hyp; e += CAP) s_hypid[e] = a.t.hyp_id[(size_t)s * MAXH + e];
    // lane c holds classes c and c + 64
    long long cnt[2][5];
    double isum[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = lane + CAP * k;
#pragma unroll
      for (int w = 0; w < 5; ++w) cnt[k][w] = c < classes ? a.t.counts[((size_t)s * classes + c) * 5 + w] : 0;
      isum[k] = c < classes ? a.t.iou_sum[(size_t)s * classes + c] : 0.0;
    }

    for (int f = 0; f < a.F && status == 0; ++f) {
      const size_t img = (size_t)s * a.F + f;
      int hc = a.counts[img], gc = a.gt_count[img];               // (both loads issued before either is waited for)
      hc = clamp_count(hc, rows);
      gc = clamp_count(gc, G);
      __syncthreads();                  // the previous frame's LDS is no longer read
      // ---- validity: lane = hypothesis row, lane = object row
      bool hv = false, ov = false, ign = false;
      int hid = 0, hcl = 0, oid = 0, ocl = 0;
      if (lane < hc) {
        const size_t r = img * rows + lane;
        const f32x4 b = {a.boxes[r * 4], a.boxes[r * 4 + 1], a.boxes[r * 4 + 2], a.boxes[r * 4 + 3]};
        hid = a.ids[r];
        hcl = a.cls[r];
        const bool box = valid_box(b);  // (ahead of the chain below: inside it the kernel measured 2 % slower, profiles/tracking_refactor_bench.txt)
        hv = a.states[r] == 2 && hid > 0 && box && hcl >= 0 && hcl < classes;
        if (hv) { s_hbox[lane][0] = (double)b[0]; s_hbox[lane][1] = (double)b[1]; s_hbox[lane][2] = (double)b[2]; s_hbox[lane][3] = (double)b[3]; }
      }
      if (lane < gc) {
        const size_t r = img * G + lane;
        const double b[4] = {a.gt_box[r * 4], a.gt_box[r * 4 + 1], a.gt_box[r * 4 + 2], a.gt_box[r * 4 + 3]};
        oid = a.gt_id[r];
        ocl = a.gt_cls[r];
        const bool box = valid_box(b);
        ov = oid > 0 && box && ocl >= 0 && ocl < classes;
        ign = (a.gt_flags[r] & 1) != 0;
        if (ov) { s_obox[lane][0] = b[0]; s_obox[lane][1] = b[1]; s_obox[lane][2] = b[2]; s_obox[lane][3] = b[3]; }
      }
      s_hid[lane] = hid; s_oid[lane] = oid; s_hcls[lane] = hcl; s_ocls[lane] = ocl;
      s_taken[lane] = -1; s_omatch[lane] = -1; s_hdrop[lane] = 0; s_hti[lane] = 0;
      __syncthreads();
      {                                 // a row whose identity a lower valid row of the frame carries is invalid
        const uint64_t hb = __ballot(hv), ob = __ballot(ov);
        bool dup = false;
        for (uint64_t m = hb; m; m &= m - 1) {
          const int r = __builtin_ctzll(m);
          dup |= r < lane && lane_value(hid, r) == hid;
        }
        hv = hv && !dup;
        dup = false;
        for (uint64_t m = ob; m; m &= m - 1) {
          const int r = __builtin_ctzll(m);
          dup |= r < lane && lane_value(oid, r) == oid;
        }
        ov = ov && !dup;
      }
      ign = ign && ov;
      const uint64_t hm = __ballot(hv), om = __ballot(ov), ignm = __ballot(ign);
      // ---- dense indices: objects before hypotheses, each in row order
      int gi = find_ids(s_objid, n_obj, oid, om & ~ignm, lane), ti = find_ids(s_hypid, n_hyp, hid, hm, lane);
      const uint64_t newo = __ballot(ov && !ign && gi < 0), newh = __ballot(hv && ti < 0);
      if (n_obj + __popcll(newo) > MAXO) status |= SQDET_MOT_STATUS_OBJECTS;
      if (n_hyp + __popcll(newh) > MAXH) status |= SQDET_MOT_STATUS_HYPOTHESES;
      if (status != 0) break;           // (uniform) the stream stops here: this frame and every later one changes nothing
      if ((newo >> lane) & 1ull) {
        gi = n_obj + rank_in(newo, lane);
        s_objid[gi] = oid;
        a.t.obj_id[(size_t)s * MAXO + gi] = oid;
        a.t.obj_cls[(size_t)s * MAXO + gi] = ocl;
      }
      if ((newh >> lane) & 1ull) {
        ti = n_hyp + rank_in(newh, lane);
        s_hypid[ti] = hid;
        a.t.hyp_id[(size_t)s * MAXH + ti] = hid;
        a.t.hyp_cls[(size_t)s * MAXH + ti] = hcl;
      }
      n_obj += __popcll(newo);
      n_hyp += __popcll(newh);
      const size_t orow = (size_t)s * MAXO + (gi < 0 ? 0 : gi);
      const bool counted = ov && !ign;                                // an object with an identity
      int last = 0, present = 0, tracked = 0, frag = 0, run = 0;
      if (counted) {
        last = a.t.obj_last[orow]; present = a.t.obj_present[orow]; tracked = a.t.obj_tracked[orow]; frag = a.t.obj_frag[orow];
        run = a.t.obj_run[orow];
      }
      // ---- 1: IoU and cost of every (valid object, valid hypothesis) pair, dealt to the lanes
      const int n_o = __popcll(om), n_h = __popcll(hm);
      list_lane(ov, om, s_olist, lane);
      list_lane(hv, hm, s_hlist, lane);
      if (hv) s_hti[lane] = ti;
      __syncthreads();
      deal_pairs(n_o, n_h, s_olist, s_hlist, lane, [&](int o, int h) {                  // box 1 the object, box 2 the hypothesis
        const double ob[4] = {s_obox[o][0], s_obox[o][1], s_obox[o][2], s_obox[o][3]};
        const double hb[4] = {s_hbox[h][0], s_hbox[h][1], s_hbox[h][2], s_hbox[h][3]};
        const double v = s_ocls[o] == s_hcls[h] ? iou(ob, hb) : 0.0;
        s_iou[o * MSTRIDE + h] = v;
        s_q[o * MSTRIDE + h] = v >= a.iou_thresh ? (int)(long long)__builtin_floor((1.0 - v) * 1048576.0) : -1;
      });
      __syncthreads();
      // ---- 2: continuity (lane = object): the hypothesis that carries the object's last id, if the pair is allowed; of several
      // objects after one hypothesis the lowest row has it
      int match = -1, cand = -1;
      uint64_t amask = 0;                                              // the hypotheses allowed with object `lane`
      if (ov) {
#pragma unroll 4
        for (uint64_t m = hm; m; m &= m - 1) {
          const int h = __builtin_ctzll(m);
          amask |= (uint64_t)(s_q[lane * MSTRIDE + h] >= 0) << h;
        }
      }
      for (uint64_t m = hm; m; m &= m - 1) {                          // (a frame's hypothesis ids differ: at most one hit)
        const int h = __builtin_ctzll(m), id_h = lane_value(hid, h);
        if (counted && last > 0 && id_h == last && ((amask >> h) & 1ull)) cand = h;
      }
      {
        const uint64_t cm = __ballot(cand >= 0);
        bool win = cand >= 0;
        for (uint64_t m = cm; m; m &= m - 1) {
          const int r = __builtin_ctzll(m), c_r = lane_value(cand, r);
          win = win && !(r < lane && c_r == cand);
        }
        if (win) { match = cand; s_taken[cand] = lane; }
      }
      __syncthreads();
      // ---- 3: the optimal assignment of what is left, compacted in order, on the square matrix of side N
      {
        const uint64_t ro = om & ~__ballot(match >= 0), rh = hm & ~__ballot(hv && s_taken[lane] >= 0);
        const int R = __popcll(ro), C = __popcll(rh), N = R > C ? R : C;
        if (R > 0 && C > 0) {
          list_lane((ro >> lane) & 1ull, ro, s_rowobj, lane);
          list_lane((rh >> lane) & 1ull, rh, s_colhyp, lane);
          __syncthreads();
          const int mycol = lane < C ? s_colhyp[lane] : -1;            // (column j is lane j)
          const int* rowobj = s_rowobj;
          const int* q = s_q;
          auto cost = [=](int i, int) -> long long {
            if (i >= R || mycol < 0) return BIG;
            const int c = q[rowobj[i] * MSTRIDE + mycol];
            return c < 0 ? BIG : (long long)c;
          };
          assign<CAP, 1>(N, N, cost, s_u, s_p, s_way, s_wv, s_wj, lane);
          if (mycol >= 0) {
            const int i = s_p[lane];
            if (i >= 0 && i < R) {
              const int o = s_rowobj[i];
              if (s_q[o * MSTRIDE + mycol] >= 0) { s_taken[mycol] = o; s_omatch[o] = mycol; }
            }
          }
          __syncthreads();
          if (match < 0) match = s_omatch[lane];
        }
      }
      // ---- 4: counts.  Lane = object: its identity's words
      int idsw = 0;
      if (ov && match >= 0) {
        if (ign) s_hdrop[match] = 1;
        else {
          const int h = s_hid[match];
          idsw = last > 0 && last != h;
          last = h;
          tracked += 1;
          if (run == 2) frag += 1;
          run = 1;
        }
      } else if (counted && run == 1) {
        run = 2;
      }
      if (counted) {
        a.t.obj_last[orow] = last; a.t.obj_present[orow] = present + 1; a.t.obj_tracked[orow] = tracked; a.t.obj_frag[orow] = frag;
        a.t.obj_run[orow] = run;
      }
      __syncthreads();
      // lane = hypothesis: the frames of its identity
      const bool hdrop = s_hdrop[lane] != 0;
      const int htaken = s_taken[lane];
      if (hv && !hdrop) a.t.hyp_frames[(size_t)s * MAXH + ti] += 1;
      // lane = object: its row of overlap, every allowed pair whose hypothesis was not dropped
      const uint64_t dropm = __ballot(hdrop);                          // (every lane votes: not inside the branch below)
      if (counted) {
        int32_t* row = a.t.overlap + ((size_t)s * MAXO + gi) * MAXH;
        for (uint64_t m = amask & ~dropm; m; m &= m - 1) row[s_hti[__builtin_ctzll(m)]] += 1;
      }
      // lane = class: the frame's objects and hypotheses in row order, read from their lanes' registers
      const double miou = ov && match >= 0 ? s_iou[lane * MSTRIDE + match] : 0.0;
      for (uint64_t m = om; m; m &= m - 1) {
        const int o = __builtin_ctzll(m), c = lane_value(ocl, o), mt = lane_value(match, o), sw = lane_value(idsw, o);
        const double v = lane_value(miou, o);
        const bool ig = (ignm >> o) & 1ull;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          if (c != lane + CAP * k) continue;
          if (ig) cnt[k][4] += mt >= 0;
          else if (mt >= 0) { cnt[k][0] += 1; isum[k] = isum[k] + v; cnt[k][3] += sw; }
          else cnt[k][1] += 1;
        }
      }
      for (uint64_t m = hm & ~__ballot(htaken >= 0); m; m &= m - 1) {
        const int c = lane_value(hcl, __builtin_ctzll(m));
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (c == lane + CAP * k) cnt[k][2] += 1;
      }
    }

#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = lane + CAP * k;
      if (c < classes) {
#pragma unroll
        for (int w = 0; w < 5; ++w) a.t.counts[((size_t)s * classes + c) * 5 + w] = cnt[k][w];
        a.t.iou_sum[(size_t)s * classes + c] = isum[k];
      }
    }
    if (lane == 0) { a.t.n_obj[s] = n_obj; a.t.n_hyp[s] = n_hyp; a.t.status[s] = status; }
  }
}

// ------------------------------------------------------------------------------------------------ evaluation
// One workgroup per stream: IDF1's global matching on the stream's overlap table, then lane = class over the identity tables.
__global__ void __launch_bounds__(EV_THREADS) mot_evaluate_kernel(const sqdet_mot_tables_t t, int classes, int64_t* result) {
  __shared__ long long s_u[MAXO], s_wv[EV_THREADS / 64];
  __shared__ int s_wj[EV_THREADS / 64];
  __shared__ int s_p[MAXH], s_way[MAXH], s_hcls[MAXH], s_hfr[MAXH];
  __shared__ int s_ocls[MAXO], s_opres[MAXO], s_otrk[MAXO], s_ofrag[MAXO], s_oidtp[MAXO];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int R = clamp_count(t.n_obj[s], MAXO), T = clamp_count(t.n_hyp[s], MAXH);      // (a loaded table is the caller's: stay inside it)
  const int C = T > R ? T : R;
  const int32_t* overlap = t.overlap + (size_t)s * MAXO * MAXH;
  for (int i = tid; i < R; i += EV_THREADS) {
    s_ocls[i] = t.obj_cls[(size_t)s * MAXO + i]; s_opres[i] = t.obj_present[(size_t)s * MAXO + i];
    s_otrk[i] = t.obj_tracked[(size_t)s * MAXO + i]; s_ofrag[i] = t.obj_frag[(size_t)s * MAXO + i];
    s_oidtp[i] = 0;
  }
  for (int j = tid; j < T; j += EV_THREADS) { s_hcls[j] = t.hyp_cls[(size_t)s * MAXH + j]; s_hfr[j] = t.hyp_frames[(size_t)s * MAXH + j]; }
  if (R > 0) {
    auto cost = [=](int i, int j) -> long long { return j < T ? -(long long)overlap[(size_t)i * MAXH + j] : 0ll; };
    assign<EV_THREADS, EV_COLS>(R, C, cost, s_u, s_p, s_way, s_wv, s_wj, tid);
    for (int j = tid; j < T; j += EV_THREADS) {
      const int i = s_p[j];
      if (i >= 0) s_oidtp[i] = overlap[(size_t)i * MAXH + j];           // (a row has one column)
    }
  }
  __syncthreads();
  for (int c = tid; c < classes; c += EV_THREADS) {
    long long frag = 0, mt = 0, pt = 0, ml = 0, idtp = 0, pres = 0, nobj = 0, hfr = 0, nhyp = 0;
    for (int i = 0; i < R; ++i) {
      if (s_ocls[i] != c) continue;
      const long long present = s_opres[i], tracked = s_otrk[i];
      frag += s_ofrag[i];
      if (5 * tracked >= 4 * present) mt += 1;
      else if (5 * tracked < present) ml += 1;
      else pt += 1;
      idtp += s_oidtp[i];
      pres += present;
      nobj += 1;
    }
    for (int j = 0; j < T; ++j) {
      if (s_hcls[j] != c) continue;
      hfr += s_hfr[j];
      nhyp += 1;
    }
    int64_t* out = result + ((size_t)s * classes + c) * KOUT;
    const int64_t* in = t.counts + ((size_t)s * classes + c) * 5;
#pragma unroll
    for (int w = 0; w < 5; ++w) out[w] = in[w];
    out[5] = frag; out[6] = mt; out[7] = pt; out[8] = ml; out[9] = idtp; out[10] = pres - idtp; out[11] = hfr - idtp; out[12] = nobj;
    out[13] = nhyp;
  }
}

int check_tables(const char* who, const sqdet_mot_tables_t* tables) {
  SQDET_REQUIRE(tables != nullptr, "%s: null tables", who);
  const sqdet_mot_tables_t& t = *tables;
  SQDET_REQUIRE(t.obj_id != nullptr && t.obj_cls != nullptr && t.obj_last != nullptr && t.obj_present != nullptr && t.obj_tracked != nullptr &&
                    t.obj_frag != nullptr && t.obj_run != nullptr && t.hyp_id != nullptr && t.hyp_cls != nullptr && t.hyp_frames != nullptr &&
                    t.n_obj != nullptr && t.n_hyp != nullptr && t.status != nullptr && t.counts != nullptr && t.iou_sum != nullptr &&
                    t.overlap != nullptr,
                "%s: null pointer in the tables", who);
  return SQDET_OK;
}

}  // namespace
}  // namespace sqdet

using namespace sqdet;

extern "C" int sqdet_mot_update(const sqdet_mot_tables_t* tables, const float* boxes, const int32_t* cls, const int32_t* counts,
                                const int32_t* det_track_id, const int32_t* det_track_state, const double* gt_box, const int32_t* gt_id,
                                const int32_t* gt_cls, const int32_t* gt_flags, const int32_t* gt_count, int streams, int frames, int rows,
                                int gt_rows, int classes, double iou_thresh, int max_workgroups, sqdet_stream_t stream) {
  if (const int rc = check_tables("sqdet_mot_update", tables)) return rc;
  SQDET_REQUIRE(boxes != nullptr && cls != nullptr && counts != nullptr && det_track_id != nullptr && det_track_state != nullptr,
                "sqdet_mot_update: null pointer among the hypotheses");
  SQDET_REQUIRE(gt_box != nullptr && gt_id != nullptr && gt_cls != nullptr && gt_flags != nullptr && gt_count != nullptr,
                "sqdet_mot_update: null pointer in the ground truth");
  SQDET_REQUIRE(streams > 0 && frames > 0 && rows > 0 && gt_rows > 0 && classes > 0,
                "sqdet_mot_update: bad sizes streams %d frames %d rows %d gt_rows %d classes %d", streams, frames, rows, gt_rows, classes);
  SQDET_REQUIRE((long long)streams * frames <= 0x7fffffffLL / SQDET_MOT_CAP, "sqdet_mot_update: %d x %d images", streams, frames);
  SQDET_REQUIRE(iou_thresh > 0.0 && iou_thresh <= 1.0, "sqdet_mot_update: iou_thresh %g (must be in (0, 1])", iou_thresh);
  SQDET_UNSUPPORTED(rows > SQDET_MOT_CAP || gt_rows > SQDET_MOT_CAP, "sqdet_mot_update: %d rows, %d objects per image (at most %d)", rows,
                    gt_rows, SQDET_MOT_CAP);
  SQDET_UNSUPPORTED(classes > SQDET_MOT_MAX_CLASSES, "sqdet_mot_update: %d classes (at most %d)", classes, SQDET_MOT_MAX_CLASSES);
  MotArgs a{};
  a.t = *tables; a.boxes = boxes; a.cls = cls; a.counts = counts; a.ids = det_track_id; a.states = det_track_state;
  a.gt_box = gt_box; a.gt_id = gt_id; a.gt_cls = gt_cls; a.gt_flags = gt_flags; a.gt_count = gt_count;
  a.S = streams; a.F = frames; a.rows = rows; a.G = gt_rows; a.classes = classes; a.iou_thresh = iou_thresh;
  hipLaunchKernelGGL(mot_update_kernel, dim3((unsigned)stream_grid(max_workgroups, streams)), dim3(CAP), 0, as_stream(stream), a);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" int sqdet_mot_evaluate(const sqdet_mot_tables_t* tables, int streams, int classes, int64_t* result_device,
                                  int64_t* host_counters, double* host_iou_sum, sqdet_stream_t stream) {
  if (const int rc = check_tables("sqdet_mot_evaluate", tables)) return rc;
  SQDET_REQUIRE(result_device != nullptr && host_counters != nullptr && host_iou_sum != nullptr, "sqdet_mot_evaluate: null pointer");
  SQDET_REQUIRE(streams > 0 && classes > 0, "sqdet_mot_evaluate: bad sizes streams %d classes %d", streams, classes);
  SQDET_UNSUPPORTED(classes > SQDET_MOT_MAX_CLASSES, "sqdet_mot_evaluate: %d classes (at most %d)", classes, SQDET_MOT_MAX_CLASSES);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(mot_evaluate_kernel, dim3((unsigned)streams), dim3(EV_THREADS), 0, st, *tables, classes, result_device);
  SQDET_CHECK_HIP(hipGetLastError());
  // staged, so that a failure leaves the host outputs alone
  const size_t nc = (size_t)streams * classes * KOUT, ni = (size_t)streams * classes;
  std::vector<int64_t> counters(nc);
  std::vector<double> iou_sum(ni);
  std::vector<int32_t> status(streams);
  SQDET_CHECK_HIP(hipMemcpyAsync(counters.data(), result_device, nc * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  SQDET_CHECK_HIP(hipMemcpyAsync(iou_sum.data(), tables->iou_sum, ni * sizeof(double), hipMemcpyDeviceToHost, st));
  SQDET_CHECK_HIP(hipMemcpyAsync(status.data(), tables->status, (size_t)streams * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  SQDET_CHECK_HIP(hipStreamSynchronize(st));
  for (int s = 0; s < streams; ++s)
    SQDET_UNSUPPORTED(status[s] != 0, "sqdet_mot_evaluate: stream %d met more than %d object or %d hypothesis identities (status %d)", s,
                      SQDET_MOT_MAX_OBJECTS, SQDET_MOT_MAX_HYPOTHESES, status[s]);
  memcpy(host_counters, counters.data(), nc * sizeof(int64_t));
  memcpy(host_iou_sum, iou_sum.data(), ni * sizeof(double));
  return SQDET_OK;
}
