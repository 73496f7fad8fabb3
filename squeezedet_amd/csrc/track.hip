// Multi-object tracking over the filtered detection rows (sqdet_track_update, sqdet_track_build_items; include/sqdet.h,
// "tracking"): the stage behind filter_prediction that gives the rows of a video or of a bank of cameras identities that last.
// The reference has nothing of the kind; the definition is the header's, restated sequentially in tests/track_reference.py.
//
// One WAVE per stream.  A stream has 64 slots and a frame at most 64 rows, so lane t IS slot t for everything a slot does
// (predict, its side of the association, update, miss, birth) and lane d IS row d for everything a row does (validity, its
// class of threshold, its side of the association, its two output words).  A slot's filter state -- 20 doubles, 6 ints, a float -- stays in its lane's
// registers over the F frames of a call and goes back to the tables once.
//
// Association.  The affinity matrix lives in LDS, one padded row per slot.  The row boxes and the predicted boxes are staged in
// LDS by their lanes, and the (live slot, valid row) pairs are dealt to the 64 lanes in turn -- an IoU is ~35 float64
// instructions with its division, and a steady scene has far fewer pairs than 64 x 64.  A greedy round is a wave-wide arg-max from both
// sides at once (greedy() below): slot lanes hold the best free row of their LDS row, row lanes the best free slot of their LDS
// column, and every pair that is each other's best is matched in the same round -- the pairs a sequential scan in the order
// (M descending, slot ascending, row ascending) keeps.  A tracking scene needs two or three rounds, not one per track.  Only
// the lanes whose cached best was just taken rescan.  Sets of rows and slots are 64-bit ballot masks, uniform over the wave.
//
// -ffp-contract=off (build.py): every operator of the header's definition is one IEEE operation, compared bit for bit.
#include "draw_items.h"
#include "stream_wave.h"

namespace sqdet {
namespace {

constexpr int CAP = SQDET_TRACK_CAP;
constexpr int MSTRIDE = CAP + 1;                   // doubles: lane t's row starts 2 banks after lane t-1's
static_assert(CAP == 64, "one slot per lane of a wave");

struct TrackArgs {
  sqdet_track_tables_t t;
  const float* boxes;
  const float* probs;
  const int32_t* cls;
  const int32_t* counts;
  int32_t* out_id;
  int32_t* out_state;
  int S, F, rows;
  sqdet_track_params_t p;
};

// The best candidate of `mask` (uniform) among base[i * STRIDE]: the largest value >= thresh, the lowest index among equals; -1 / -1 if
// none.  Four set bits at a time, so that four LDS reads are in flight (a short tail repeats its last index: harmless under the
// strict comparison).
template <int STRIDE>
__device__ __forceinline__ void scan(const double* base, uint64_t mask, double thresh, double& best, int& besti) {
  best = -1.0;
  besti = -1;
  for (uint64_t m = mask; m;) {
    int i[4];
    i[0] = __builtin_ctzll(m);
    m &= m - 1;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      i[k] = m ? __builtin_ctzll(m) : i[k - 1];
      m &= m - 1;                                                // (0 stays 0)
    }
    double v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = base[i[k] * STRIDE];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (v[k] >= thresh && v[k] > best) { best = v[k]; besti = i[k]; }
  }
}

// One stage of the greedy association.  slot_in: this lane's slot takes part; rowsm: the stage's rows (uniform), on return those
// still free.  Returns the lane's row, -1 if its slot stays unmatched.
//
// The sequential rule -- take the free pair that is first in the order (M descending, slot ascending, row ascending) while its
// M >= thresh -- keeps exactly the pairs that are, at some point, first in that order among all free pairs sharing their slot
// or their row: such a pair cannot lose either end to an earlier pair, and once it is removed the argument repeats on the rest.
// So a round matches ALL pairs that are each other's best at once: slot lanes hold the best free row of their LDS row, row lanes
// the best free slot of their LDS column, both in that order, and exchange them through LDS.  The first free pair of the whole
// order is always mutual, so a round without a match ends the stage.  Only lanes whose cached best was just taken rescan.
__device__ __forceinline__ int greedy(const double* s_M, int* s_bestrow, int* s_bestslot, bool slot_in, uint64_t& rowsm, double thresh,
                                      int lane) {
  uint64_t slotsm = __ballot(slot_in);
  bool row_in = (rowsm >> lane) & 1ull;
  double sb = -1.0, rb = -1.0;
  int sd = -1, rt = -1, match = -1;
  if (slotsm == 0 || rowsm == 0) return match;
  if (slot_in) scan<1>(s_M + lane * MSTRIDE, rowsm, thresh, sb, sd);
  if (row_in) scan<MSTRIDE>(s_M + lane, slotsm, thresh, rb, rt);
  while (true) {
    s_bestrow[lane] = slot_in ? sd : -1;
    s_bestslot[lane] = row_in ? rt : -1;
    __syncthreads();
    const bool sm = slot_in && sd >= 0 && s_bestslot[sd] == lane;
    const bool rm = row_in && rt >= 0 && s_bestrow[rt] == lane;
    __syncthreads();                                             // read before the next round writes
    const uint64_t tslots = __ballot(sm), trows = __ballot(rm);
    if (tslots == 0) break;
    slotsm &= ~tslots;
    rowsm &= ~trows;
    if (sm) { match = sd; slot_in = false; }
    else if (slot_in && sd >= 0 && ((trows >> sd) & 1ull)) scan<1>(s_M + lane * MSTRIDE, rowsm, thresh, sb, sd);
    if (rm) row_in = false;
    else if (row_in && rt >= 0 && ((tslots >> rt) & 1ull)) scan<MSTRIDE>(s_M + lane, slotsm, thresh, rb, rt);
  }
  return match;
}

__global__ void __launch_bounds__(CAP) track_kernel(const TrackArgs a) {
  __shared__ double s_M[CAP * MSTRIDE];
  __shared__ double s_box[CAP][4], s_pbox[CAP][4];
  __shared__ float s_prob[CAP];
  __shared__ int s_cls[CAP], s_id[CAP], s_st[CAP], s_birth[CAP], s_bestrow[CAP], s_bestslot[CAP], s_pcls[CAP], s_live[CAP], s_valid[CAP];
  const int lane = threadIdx.x, rows = a.rows;
  const sqdet_track_params_t& p = a.p;

  for (int s = blockIdx.x; s < a.S; s += gridDim.x) {
    const size_t slot = (size_t)s * CAP + lane;
    double xp[4], xv[4], pp[4], pv[4], vv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      xp[c] = a.t.x[slot * 8 + c * 2]; xv[c] = a.t.x[slot * 8 + c * 2 + 1];
      pp[c] = a.t.P[slot * 12 + c * 3]; pv[c] = a.t.P[slot * 12 + c * 3 + 1]; vv[c] = a.t.P[slot * 12 + c * 3 + 2];
    }
    int cls = a.t.cls[slot], id = a.t.id[slot], state = a.t.state[slot], hits = a.t.hits[slot], miss = a.t.miss[slot], age = a.t.age[slot];
    float score = a.t.score[slot];
    int next_id = a.t.next_id[s], dropped = a.t.dropped[s];

    for (int f = 0; f < a.F; ++f) {
      const size_t img = (size_t)s * a.F + f;
      const int count = clamp_count(a.counts[img], rows);                                          // 1
      __syncthreads();                  // the previous frame's LDS is no longer read
      // ---- 3: rows (lane = row)
      bool high = false, low = false;
      if (lane < count) {
        const size_t r = img * rows + lane;
        const f32x4 b = {a.boxes[r * 4], a.boxes[r * 4 + 1], a.boxes[r * 4 + 2], a.boxes[r * 4 + 3]};
        const float pr = a.probs[r];
        if (valid_box(b) && finite_f(pr)) {
          high = (double)pr > p.high_thresh;
          low = !high && (double)pr > p.low_thresh;
          s_box[lane][0] = (double)b[0]; s_box[lane][1] = (double)b[1]; s_box[lane][2] = (double)b[2]; s_box[lane][3] = (double)b[3];
          s_prob[lane] = pr;
          s_cls[lane] = a.cls[r];
        }
      }
      s_id[lane] = -1;
      s_st[lane] = 0;
      const uint64_t highm = __ballot(high), lowm = __ballot(low);
      // ---- 2: predict (lane = slot)
      const bool live = state != 0;
      double box[4] = {0.0, 0.0, 1.0, 1.0};
      if (live) {
        const double h = dmax(xp[3], 1.0);
        const double qp = (p.w_pos * h) * (p.w_pos * h), qv = (p.w_vel * h) * (p.w_vel * h);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          xp[c] = xp[c] + xv[c];
          const double npp = ((pp[c] + pv[c]) + (pv[c] + vv[c])) + qp;
          pv[c] = pv[c] + vv[c];
          vv[c] = vv[c] + qv;
          pp[c] = npp;
        }
        age += 1;
        box[0] = xp[0]; box[1] = xp[1]; box[2] = dmax(xp[2], 1.0); box[3] = dmax(xp[3], 1.0);
      }
      // ---- 4: M over (live slot, valid row), the pairs dealt to the lanes: 20 tracks x 40 rows are 13 IoUs per lane, not 40
      const uint64_t livem = __ballot(live), validm = highm | lowm;
      const int n_live = __popcll(livem), n_valid = __popcll(validm);
      if (live) {
        s_pbox[lane][0] = box[0]; s_pbox[lane][1] = box[1]; s_pbox[lane][2] = box[2]; s_pbox[lane][3] = box[3];
        s_pcls[lane] = cls;
      }
      list_lane(live, livem, s_live, lane);
      list_lane((validm >> lane) & 1ull, validm, s_valid, lane);
      __syncthreads();                  // the rows, the predictions and the two lists are staged
      deal_pairs(n_live, n_valid, s_live, s_valid, lane, [&](int t, int d) {           // box 1 the prediction, box 2 the row
        const double pb[4] = {s_pbox[t][0], s_pbox[t][1], s_pbox[t][2], s_pbox[t][3]};
        const double z[4] = {s_box[d][0], s_box[d][1], s_box[d][2], s_box[d][3]};
        s_M[t * MSTRIDE + d] = s_cls[d] == s_pcls[t] ? iou(pb, z) : 0.0;
      });
      __syncthreads();                  // M is read across lanes: a row lane scans its column
      uint64_t free_high = highm, free_low = lowm;
      int match = greedy(s_M, s_bestrow, s_bestslot, live, free_high, p.iou_thresh, lane);
      if (free_low != 0) {
        const int m2 = greedy(s_M, s_bestrow, s_bestslot, live && match < 0 && state == 2, free_low, p.iou_thresh, lane);
        match = match < 0 ? m2 : match;
      }
      // ---- 6 / 7
      if (match >= 0) {
        const double h = dmax(xp[3], 1.0);
        const double r = (p.w_pos * h) * (p.w_pos * h);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double y = s_box[match][c] - xp[c];
          const double sd = pp[c] + r;
          const double kp = pp[c] / sd, kv = pv[c] / sd;
          xp[c] = xp[c] + kp * y;
          xv[c] = xv[c] + kv * y;
          const double npp = pp[c] - kp * pp[c], npv = pv[c] - kp * pv[c], nvv = vv[c] - kv * pv[c];
          pp[c] = npp; pv[c] = npv; vv[c] = nvv;
        }
        hits += 1;
        miss = 0;
        score = s_prob[match];
        if (state == 1 && hits >= p.min_hits) state = 2;
        s_id[match] = id;               // (a row has at most one slot)
        s_st[match] = state;
      } else if (live) {
        miss += 1;
        if (state == 1 || miss > p.max_age) state = 0;
      }
      // ---- 8: the k-th unmatched high row takes the k-th free slot
      const uint64_t freem = __ballot(state == 0);
      const int n_free = __popcll(freem), n_new = __popcll(free_high);
      list_lane((free_high >> lane) & 1ull, free_high, s_birth, lane);
      __syncthreads();
      const int rank = rank_in(freem, lane);
      if (state == 0 && rank < n_new) {
        const int d = s_birth[rank];
        const double h = dmax(s_box[d][3], 1.0);
        const double ka = (2.0 * p.w_pos) * h, kb = (10.0 * p.w_vel) * h;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          xp[c] = s_box[d][c]; xv[c] = 0.0;
          pp[c] = ka * ka; pv[c] = 0.0; vv[c] = kb * kb;
        }
        cls = s_cls[d];
        score = s_prob[d];
        id = next_id + rank;
        hits = 1; miss = 0; age = 1;
        state = p.min_hits <= 1 ? 2 : 1;
        s_id[d] = id;
        s_st[d] = state;
      }
      const int born = n_new < n_free ? n_new : n_free;
      next_id += born;
      dropped += n_new - born;
      __syncthreads();
      // ---- 9: the two output words of row `lane`
      if (lane < rows) {
        a.out_id[img * rows + lane] = s_id[lane];
        a.out_state[img * rows + lane] = s_st[lane];
      }
    }

#pragma unroll
    for (int c = 0; c < 4; ++c) {
      a.t.x[slot * 8 + c * 2] = xp[c]; a.t.x[slot * 8 + c * 2 + 1] = xv[c];
      a.t.P[slot * 12 + c * 3] = pp[c]; a.t.P[slot * 12 + c * 3 + 1] = pv[c]; a.t.P[slot * 12 + c * 3 + 2] = vv[c];
    }
    a.t.cls[slot] = cls; a.t.id[slot] = id; a.t.state[slot] = state; a.t.hits[slot] = hits; a.t.miss[slot] = miss; a.t.age[slot] = age;
    a.t.score[slot] = score;
    if (lane == 0) { a.t.next_id[s] = next_id; a.t.dropped[s] = dropped; }
  }
}

// ------------------------------------------------------------------------------------------------ item builder
// build_items_kernel's rule (draw_items.h) for the rows of confirmed tracks: "<name> #<id>", one colour per id.
struct TrackRule {
  const float* boxes;
  const int32_t* ids;
  const int32_t* states;
  const unsigned char* palette;
  int palette_len;
  __device__ bool keep(size_t row) const { return states[row] == 2 && ids[row] > 0; }
  __device__ void corners(size_t row, double v[4]) const { corners_of(boxes + row * 4, false, v); }
  __device__ uint32_t colour(size_t row, int, bool) const {
    const unsigned char* q = palette + (size_t)(ids[row] % palette_len) * 3;
    return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
  }
  __device__ void label(LabelWriter& w, const ItemArgs&, size_t row) const {
    w.puts(" #");
    w.decimal(ids[row]);
  }
};

}  // namespace
}  // namespace sqdet

using namespace sqdet;

extern "C" int sqdet_track_update(const sqdet_track_tables_t* tables, const float* boxes, const float* probs, const int32_t* cls,
                                  const int32_t* counts, int streams, int frames, int rows, const sqdet_track_params_t* params,
                                  int32_t* det_track_id, int32_t* det_track_state, int max_workgroups, sqdet_stream_t stream) {
  SQDET_REQUIRE(tables != nullptr && params != nullptr, "sqdet_track_update: null tables / params");
  const sqdet_track_tables_t& t = *tables;
  SQDET_REQUIRE(t.x != nullptr && t.P != nullptr && t.cls != nullptr && t.id != nullptr && t.state != nullptr && t.hits != nullptr &&
                    t.miss != nullptr && t.age != nullptr && t.score != nullptr && t.next_id != nullptr && t.dropped != nullptr,
                "sqdet_track_update: null pointer in the tables");
  SQDET_REQUIRE(boxes != nullptr && probs != nullptr && cls != nullptr && counts != nullptr && det_track_id != nullptr && det_track_state != nullptr,
                "sqdet_track_update: null pointer");
  SQDET_REQUIRE(streams > 0 && frames > 0 && rows > 0, "sqdet_track_update: bad sizes streams %d frames %d rows %d", streams, frames, rows);
  SQDET_REQUIRE((long long)streams * frames <= 0x7fffffffLL / SQDET_TRACK_CAP, "sqdet_track_update: %d x %d images", streams, frames);
  const sqdet_track_params_t& p = *params;
  const double lim = __builtin_inf();
  SQDET_REQUIRE(p.iou_thresh > 0.0 && p.iou_thresh < lim, "sqdet_track_update: iou_thresh %g (must be positive and finite)", p.iou_thresh);
  SQDET_REQUIRE(__builtin_fabs(p.high_thresh) < lim && __builtin_fabs(p.low_thresh) < lim && __builtin_fabs(p.w_pos) < lim && __builtin_fabs(p.w_vel) < lim,
                "sqdet_track_update: a threshold or weight is not finite");
  SQDET_REQUIRE(p.min_hits >= 0 && p.max_age >= 0, "sqdet_track_update: min_hits %d max_age %d", p.min_hits, p.max_age);
  SQDET_UNSUPPORTED(rows > SQDET_TRACK_CAP, "sqdet_track_update: %d rows per image (at most %d)", rows, SQDET_TRACK_CAP);
  TrackArgs a{};
  a.t = t; a.boxes = boxes; a.probs = probs; a.cls = cls; a.counts = counts; a.out_id = det_track_id; a.out_state = det_track_state;
  a.S = streams; a.F = frames; a.rows = rows; a.p = p;
  hipLaunchKernelGGL(track_kernel, dim3((unsigned)stream_grid(max_workgroups, streams)), dim3(CAP), 0, as_stream(stream), a);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" int sqdet_track_build_items(const float* boxes, const float* probs, const int32_t* cls, const int32_t* counts,
                                       const int32_t* det_track_id, const int32_t* det_track_state, int n, int rows, double plot_thresh,
                                       const unsigned char* names, int classes, const unsigned char* palette, int palette_len, int anchor,
                                       void* items, int32_t* item_counts, int cap, sqdet_stream_t stream) {
  SQDET_REQUIRE(boxes != nullptr && probs != nullptr && cls != nullptr && counts != nullptr && det_track_id != nullptr && det_track_state != nullptr &&
                    names != nullptr && palette != nullptr && items != nullptr && item_counts != nullptr,
                "sqdet_track_build_items: null pointer");
  SQDET_REQUIRE(n > 0 && rows > 0 && classes > 0 && palette_len > 0 && cap > 0,
                "sqdet_track_build_items: bad sizes n %d rows %d classes %d palette %d cap %d", n, rows, classes, palette_len, cap);
  ItemArgs a{};
  a.probs = probs; a.cls = cls; a.counts = counts; a.names = names; a.items = reinterpret_cast<unsigned char*>(items);
  a.item_counts = item_counts; a.rows = rows; a.classes = classes; a.anchor = anchor; a.cap = cap; a.plot_thresh = plot_thresh;
  return build_items("sqdet_track_build_items", a, TrackRule{boxes, det_track_id, det_track_state, palette, palette_len}, n, stream);
}
