// The device detection table of the evaluators (include/sqdet.h, "Detection table") and what kitti_eval.hip,
// voc_eval.hip and coco_eval.hip do with it: the ingest of filter rows, the per-image row gather, the wave and block helpers of their
// matchers and rank kernels, the class lists of the VOC and COCO metrics, and the host checks and tails of their entry points.
// Build with -ffp-contract=off: the row formats' arithmetic is compared bit for bit with what the host programs print.
#pragma once
#include "common.h"
#include "round_decimal.h"

namespace sqdet {
namespace {

constexpr int DT_MAX_ROWS = SQDET_KITTI_MAX_DETECTIONS;  // detection rows per image
constexpr int DT_MAX_GT = SQDET_KITTI_MAX_GROUNDTRUTH;   // ground-truth rows per image
constexpr int DT_RANK = 256;                             // threads of a count_before block
static_assert(DT_MAX_ROWS == SQDET_VOC_MAX_DETECTIONS && DT_MAX_GT == SQDET_VOC_MAX_GROUNDTRUTH, "one table, one set of limits");
static_assert(DT_MAX_ROWS == SQDET_COCO_MAX_DETECTIONS && DT_MAX_GT == SQDET_COCO_MAX_GROUNDTRUTH, "one table, one set of limits");

struct DetTable {
  double* box;       // [num_images, cap, 4] x1, y1, x2, y2
  double* score;     // [num_images, cap]
  int32_t* cls;      // [num_images, cap]
  int32_t* count;    // [num_images] rows of the image
  int32_t* status;   // [2]: sticky SQDET_EINVAL of a rejected ingest, the last ingest's verdict (may be NULL where only read back)
  int num_images, cap;
};

// The table of an entry point that only reads it (the scoring kernels never write through these pointers).
inline DetTable read_only_table(const double* box, const double* score, const int32_t* cls, const int32_t* count,
                                const int32_t* status, int num_images, int cap) {
  return DetTable{const_cast<double*>(box), const_cast<double*>(score), const_cast<int32_t*>(cls), const_cast<int32_t*>(count),
                  const_cast<int32_t*>(status), num_images, cap};
}

// ------------------------------------------------------------------------------------------------------ ingest
// What a detection file carries for one filter row (cx, cy, w, h in float32; x and y scale): x1, y1, x2, y2 as doubles.
struct KittiRow {  // double arithmetic, rounded as '%.2f'
  __device__ __forceinline__ void operator()(const float* b, double sx, double sy, double* o) const {
    const double cx = (double)b[0] / sx, cy = (double)b[1] / sy, w = (double)b[2] / sx, h = (double)b[3] / sy;
    o[0] = round_decimal(cx - w / 2, 100.0);
    o[1] = round_decimal(cy - h / 2, 100.0);
    o[2] = round_decimal(cx + w / 2, 100.0);
    o[3] = round_decimal(cy + h / 2, 100.0);
  }
  __device__ __forceinline__ double score(float p) const { return round_decimal((double)p, 1000.0); }  // '%.3f'
};

// float32 arithmetic up to the '+ 1', as NumPy's on the float32 rows (eval.py:83-91, pascal_voc.py:107-108), rounded as '{:.1f}'
struct VocRow {
  __device__ __forceinline__ void operator()(const float* b, double scale_x, double scale_y, double* o) const {
    const float sx = (float)scale_x, sy = (float)scale_y;
    const float cx = b[0] / sx, cy = b[1] / sy, w = b[2] / sx, h = b[3] / sy;
    const float x1 = cx - w / 2.0f, y1 = cy - h / 2.0f, x2 = cx + w / 2.0f, y2 = cy + h / 2.0f;
    o[0] = round_decimal((double)(x1 + 1.0f), 10.0);
    o[1] = round_decimal((double)(y1 + 1.0f), 10.0);
    o[2] = round_decimal((double)(x2 + 1.0f), 10.0);
    o[3] = round_decimal((double)(y2 + 1.0f), 10.0);
  }
  __device__ __forceinline__ double score(float p) const { return round_decimal((double)p, 1000.0); }  // '{:.3f}'
};

// COCO results carry x, y, w, h: double arithmetic, nothing rounded (coco_eval.hip), the score widened as it is
struct CocoRow {
  __device__ __forceinline__ void operator()(const float* b, double sx, double sy, double* o) const {
    const double cx = (double)b[0] / sx, cy = (double)b[1] / sy, w = (double)b[2] / sx, h = (double)b[3] / sy;
    o[0] = cx - w / 2;
    o[1] = cy - h / 2;
    o[2] = w;
    o[3] = h;
  }
  __device__ __forceinline__ double score(float p) const { return (double)p; }
};

// One block: is every count of this call in [0, max_out] and every class of its rows in [0, classes)?  status[1] = this
// call's verdict (the write kernel reads it); a bad call also sets status[0] (sticky until the table is reset).
__global__ void __launch_bounds__(256) ingest_check_kernel(const int32_t* __restrict__ cls, const int32_t* __restrict__ count,
                                                           int n, int max_out, int classes, int32_t* status) {
  __shared__ int bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  int b = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int c = count[i];
    if (c < 0 || c > max_out) b = 1;
  }
  for (size_t r = threadIdx.x; r < (size_t)n * max_out; r += blockDim.x) {
    const int i = (int)(r / max_out), j = (int)(r % max_out);
    const int c = count[i];
    if (j < c && c <= max_out && (cls[r] < 0 || cls[r] >= classes)) b = 1;
  }
  if (b) atomicOr(&bad, 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    status[1] = bad;
    if (bad) status[0] = SQDET_EINVAL;
  }
}

// One wave per image: rows in file order (class-major, then filter order), each value as the detection files carry it
// (Row: the coordinates and the score).
template <class Row>
__global__ void __launch_bounds__(64) ingest_kernel(const float* __restrict__ boxes, const float* __restrict__ probs,
                                                    const int32_t* __restrict__ cls, const int32_t* __restrict__ count,
                                                    const double* __restrict__ scales, int max_out, int image_offset, DetTable t) {
  if (t.status[1]) return;
  const int i = blockIdx.x;
  const int n = count[i];
  const size_t src = (size_t)i * max_out, dst = (size_t)(image_offset + i) * t.cap;
  const double sx = scales ? scales[2 * i] : 1.0, sy = scales ? scales[2 * i + 1] : 1.0;
  for (int j = threadIdx.x; j < n; j += 64) {
    const int c = cls[src + j];
    int pos = 0;  // rows of smaller classes, then rows of the same class before j
    for (int k = 0; k < n; ++k) {
      const int ck = cls[src + k];
      pos += (ck < c) || (ck == c && k < j);
    }
    Row()(boxes + (src + j) * 4, sx, sy, t.box + (dst + pos) * 4);
    t.score[dst + pos] = Row().score(probs[src + j]);
    t.cls[dst + pos] = c;
  }
  if (threadIdx.x == 0) t.count[image_offset + i] = n;
}

// The body of sqdet_<who>: n images of filter rows into table images [image_offset, image_offset + n).
template <class Row>
int ingest_rows(const char* who, const float* boxes, const float* probs, const int32_t* cls, const int32_t* count,
                const double* scales, int n, int max_out, int classes, int max_classes, const DetTable& t, int image_offset,
                sqdet_stream_t stream) {
  SQDET_REQUIRE(boxes && probs && cls && count && t.box && t.score && t.cls && t.count && t.status, "%s: null pointer", who);
  SQDET_REQUIRE(n >= 0 && max_out > 0 && t.cap > 0 && t.num_images >= 0 && classes > 0, "%s: bad dims", who);
  SQDET_UNSUPPORTED(classes > max_classes, "%s: %d classes (limit %d)", who, classes, max_classes);
  SQDET_UNSUPPORTED(t.cap > DT_MAX_ROWS, "%s: %d rows per image (limit %d)", who, t.cap, DT_MAX_ROWS);
  SQDET_UNSUPPORTED(max_out > t.cap, "%s: %d filter rows per image, the table holds %d", who, max_out, t.cap);
  SQDET_REQUIRE(image_offset >= 0 && (long long)image_offset + n <= t.num_images, "%s: images [%d, %lld) outside the table's %d", who,
                image_offset, (long long)image_offset + n, t.num_images);
  if (n == 0) return SQDET_OK;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ingest_check_kernel, dim3(1), dim3(256), 0, st, cls, count, n, max_out, classes, t.status);
  hipLaunchKernelGGL(ingest_kernel<Row>, dim3((unsigned)n), dim3(64), 0, st, boxes, probs, cls, count, scales, max_out, image_offset, t);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

// The tail of sqdet_<who> (an evaluate call): the workspace header and the table's status to the host, ONE synchronisation,
// then the two failures every metric shares.  Header: a struct with an `error` field whose bit 0 says "an image over the limits".
template <class Header>
int read_back(const char* who, const Header* header, const DetTable& t, int classes, hipStream_t st, Header* host) {
  int32_t st_host[2] = {0, 0};
  SQDET_CHECK_HIP(hipMemcpyAsync(host, header, sizeof(Header), hipMemcpyDeviceToHost, st));
  if (t.status) SQDET_CHECK_HIP(hipMemcpyAsync(st_host, t.status, sizeof(st_host), hipMemcpyDeviceToHost, st));
  SQDET_CHECK_HIP(hipStreamSynchronize(st));
  SQDET_REQUIRE(st_host[0] == 0, "%s: the detection table holds a rejected ingest (negative or over-capacity count, "
                "or a class outside 0..%d); reset it", who, classes - 1);
  SQDET_UNSUPPORTED(host->error & 1, "%s: an image has more than %d ground-truth or %d detection rows", who, DT_MAX_GT, t.cap);
  return SQDET_OK;
}

// ------------------------------------------------------------------------------------- per-image, one wave of 64
// Are an image's row counts within what the kernels' LDS arrays and the table hold?
__device__ __forceinline__ bool rows_ok(int ngt, int nrow, int cap) { return ngt >= 0 && ngt <= DT_MAX_GT && nrow >= 0 && nrow <= cap; }

// Are the image's row counts within the limits (and its ground-truth rows inside the arrays)?  An image that is not is
// scored as empty by every kernel, so that every offset stays inside the workspace; the call then fails.
__device__ __forceinline__ bool image_ok(int img, const DetTable& t, int num_gt, const int32_t* __restrict__ gt_off, int* g0, int* ngt,
                                         int* nrow) {
  *g0 = gt_off[img];
  *ngt = gt_off[img + 1] - *g0;
  *nrow = t.count[img];
  return rows_ok(*ngt, *nrow, t.cap) && *g0 >= 0 && (long long)*g0 + *ngt <= num_gt;
}

__device__ __forceinline__ uint64_t lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// Ballot compaction, order kept: put(j, p) for every j in [0, n) with keep(j), p = the number of kept rows before j.
// Returns the number kept.  All 64 lanes call it.
template <class Keep, class Put>
__device__ __forceinline__ int wave_compact(int n, Keep keep, Put put) {
  const int lane = threadIdx.x;
  int kept = 0;
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int j = j0 + lane;
    const bool mine = j < n && keep(j);
    const uint64_t m = __ballot(mine);
    if (mine) put(j, kept + __popcll(m & lanes_below()));
    kept += __popcll(m);
  }
  return kept;
}

// The rows of class c among image img's first nrow, table order kept, into the LDS arrays box / score.  Returns their number.
__device__ __forceinline__ int gather_class_rows(const DetTable& t, int img, int c, int nrow, double (*box)[4], double* score) {
  const size_t r0 = (size_t)img * t.cap;
  return wave_compact(
      nrow, [&](int j) { return t.cls[r0 + j] == c; },
      [&](int j, int p) {
        const double* b = t.box + (r0 + j) * 4;
        for (int q = 0; q < 4; ++q) box[p][q] = b[q];
        score[p] = t.score[r0 + j];
      });
}

// Every lane's candidate (idx < 0: none) -> in every lane the one of greatest `best`, the lowest index among equals.
__device__ __forceinline__ void wave_best_lowest_index(double& best, int& idx) {
  for (int off = 32; off > 0; off >>= 1) {
    const double ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(idx, off);
    if (oi >= 0 && (idx < 0 || ob > best || (ob == best && oi < idx))) {
      best = ob;
      idx = oi;
    }
  }
}

// Its sibling: the one of greatest `best`, the HIGHEST index among equals (a walk that takes `>=` ends on the last one).
__device__ __forceinline__ void wave_best_highest_index(double& best, int& idx) {
  for (int off = 32; off > 0; off >>= 1) {
    const double ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(idx, off);
    if (oi >= 0 && (idx < 0 || ob > best || (ob == best && oi > idx))) {
      best = ob;
      idx = oi;
    }
  }
}

// order[r] = the row of rank r by descending score, equal scores in row order (LDS arrays, n rows).  A NaN score has no
// rank: it writes nothing, and the slots no row claims keep the in-range index they start with.  Synchronises the block
// before (the scores must be written) and after.
__device__ __forceinline__ void stable_rank_desc(const double* score, int* order, int n) {
  for (int j = threadIdx.x; j < n; j += 64) order[j] = j;
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += 64) {
    const double s = score[j];
    int r = 0;
    for (int k = 0; k < n; ++k) r += score[k] > s || (score[k] == s && k < j);
    if (s == s) order[r] = j;
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------ rank, blocks of DT_RANK
struct Sum {
  template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct Max {
  template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; }
};

// Inclusive scan (Op: Sum or Max) over the block's DT_RANK threads (Hillis-Steele in LDS); buf[DT_RANK - 1] is the total
// until the next call.  Max is exact and integer sums are order-free, so the association order changes no bit.
template <class Op, class T>
__device__ __forceinline__ T block_scan_incl(T v, T* buf) {
  const int t = threadIdx.x;
  __syncthreads();
  buf[t] = v;
  __syncthreads();
  for (int off = 1; off < DT_RANK; off <<= 1) {
    const T x = buf[t >= off ? t - off : t];
    __syncthreads();
    if (t >= off) buf[t] = Op()(x, buf[t]);
    __syncthreads();
  }
  return buf[t];
}

// Against all n values of v (read through the LDS tile, DT_RANK at a time): how many are greater than e, equal to it, and
// equal to it at an index below e_idx.  Every thread of the block calls it.
struct Before {
  int greater, equal, equal_before;
};
__device__ __forceinline__ Before count_before(const double* __restrict__ v, int n, double e, int e_idx, double* tile) {
  Before b = {0, 0, 0};
  for (int t0 = 0; t0 < n; t0 += DT_RANK) {
    __syncthreads();
    if (t0 + (int)threadIdx.x < n) tile[threadIdx.x] = v[t0 + threadIdx.x];
    __syncthreads();
    const int m = n - t0 < DT_RANK ? n - t0 : DT_RANK;
    for (int q = 0; q < m; ++q) {
      const double x = tile[q];
      b.greater += x > e;
      b.equal += x == e;
      b.equal_before += x == e && t0 + q < e_idx;
    }
  }
  return b;
}

// ------------------------------------------------------------------------------------------------- class lists
// What voc_eval.hip and coco_eval.hip regroup the table into: class c owns [class_offset(c), class_offset(c) + ndet[c]) of
// a metric's per-row arrays; inside it (image, class) segments follow each other in image order, so a segment starts at
// class_offset(c) + base[c][img].  This section is the only code that knows the layout.
struct ClassLists {
  int* cnt;   // [C, N] rows of the class in the image
  int* base;  // [C, N] exclusive prefix of cnt over the images
  int* ndet;  // [C] rows of the class (in the metric's workspace header)
  int num_images;
};

__device__ __forceinline__ int class_offset(const int* ndet, int c) {
  int o = 0;
  for (int k = 0; k < c; ++k) o += ndet[k];
  return o;
}

// The count kernels' table half, one wave: image img's first nrow rows per class, added to the LDS counters nd[classes].
__device__ __forceinline__ void count_class_rows(const DetTable& t, int img, int nrow, int classes, int* nd) {
  const size_t r0 = (size_t)img * t.cap;
  for (int j = threadIdx.x; j < nrow; j += 64) {
    const int c = t.cls[r0 + j];
    if (c >= 0 && c < classes) atomicAdd(&nd[c], 1);
  }
}

// One block per class: cnt -> base and ndet[c], DT_RANK images at a time with the running total carried.
__global__ void __launch_bounds__(DT_RANK) class_scan_kernel(ClassLists L) {
  __shared__ int buf[DT_RANK];
  const int c = blockIdx.x, t = threadIdx.x;
  const size_t row = (size_t)c * L.num_images;
  int carry = 0;
  for (int i0 = 0; i0 < L.num_images; i0 += DT_RANK) {
    const int i = i0 + t;
    const int v = i < L.num_images ? L.cnt[row + i] : 0;
    const int incl = block_scan_incl<Sum>(v, buf);
    if (i < L.num_images) L.base[row + i] = carry + incl - v;
    carry += buf[DT_RANK - 1];
  }
  if (t == 0) L.ndet[c] = carry;
}

// The matchers' prologue for (image, class), one wave: the class's rows of the image in the LDS arrays box / score and
// their order by descending score (stable in table order).  False for an image over the limits or an empty segment.
// Synchronises the block before it returns true.
struct Segment {
  int g0, ngt;  // the image's ground-truth rows
  int rows;     // the segment's rows in the class's list
  int nd;       // the class's rows of the image in the LDS arrays
  size_t out;   // where the segment starts in the per-row arrays
};
__device__ __forceinline__ bool class_segment(const DetTable& t, const ClassLists& L, int img, int c, int num_gt,
                                              const int32_t* __restrict__ gt_off, double (*box)[4], double* score, int* order,
                                              Segment* s) {
  int nrow;
  if (!image_ok(img, t, num_gt, gt_off, &s->g0, &s->ngt, &nrow)) return false;
  s->rows = L.cnt[(size_t)c * L.num_images + img];
  if (s->rows == 0) return false;
  s->nd = gather_class_rows(t, img, c, nrow, box, score);
  stable_rank_desc(score, order, s->nd);
  s->out = (size_t)class_offset(L.ndet, c) + L.base[(size_t)c * L.num_images + img];
  return true;
}

// The rank kernels' body, blocks of DT_RANK over (rows, classes): each row's position in its class's order -- score
// descending, then the order of the class's list -- by counting its predecessors against LDS tiles of the list;
// put(from, to) then moves the row's payload there (indices into the per-row arrays).  A NaN score has no position.
template <class Put>
__device__ __forceinline__ void rank_class_rows(const int* ndet, const double* __restrict__ cscore, Put put) {
  __shared__ double tile[DT_RANK];
  const int c = blockIdx.y, n = ndet[c];
  if ((int)(blockIdx.x * DT_RANK) >= n) return;
  const size_t off = class_offset(ndet, c);
  const int e_idx = blockIdx.x * DT_RANK + threadIdx.x;
  const double e = e_idx < n ? cscore[off + e_idx] : 0.0;
  const Before b = count_before(cscore + off, n, e, e_idx, tile);
  if (e_idx >= n || !(e == e)) return;
  put(off + e_idx, off + b.greater + b.equal_before);
}

// ---------------------------------------------------------------------------------------------- host: workspace, checks
// A running offset into a workspace: take<T>(n) aligns it for T (or to `align` bytes) and steps over n values.
struct Carver {
  char* p;
  size_t o = 0;
  template <class T>
  T* take(size_t n, size_t align = alignof(T)) {
    o = (o + align - 1) & ~(align - 1);
    T* r = reinterpret_cast<T*>(p + o);
    o += n * sizeof(T);
    return r;
  }
};

// The checks every sqdet_<who> that scores the table's class lists shares.  pointers / gt_pointers: are the entry
// point's other pointers (its ground-truth arrays, where num_gt > 0) there?
inline int check_scoring_args(const char* who, const DetTable& t, const void* gt_offsets, const void* workspace, bool pointers,
                              bool gt_pointers, int num_gt, int classes, int max_classes) {
  SQDET_REQUIRE(t.box && t.score && t.cls && t.count && gt_offsets && workspace && pointers, "%s: null pointer", who);
  SQDET_REQUIRE(t.num_images > 0 && t.cap > 0 && num_gt >= 0 && classes > 0, "%s: bad dims", who);
  SQDET_REQUIRE(num_gt == 0 || gt_pointers, "%s: null ground-truth pointer", who);
  SQDET_UNSUPPORTED(classes > max_classes, "%s: %d classes (limit %d)", who, classes, max_classes);
  SQDET_UNSUPPORTED(t.cap > DT_MAX_ROWS, "%s: %d rows per image (limit %d)", who, t.cap, DT_MAX_ROWS);
  SQDET_UNSUPPORTED((long long)t.num_images * t.cap > 0x7fffffffLL, "%s: %d images of %d rows: more than 2^31 table rows", who,
                    t.num_images, t.cap);
  return SQDET_OK;
}

}  // namespace
}  // namespace sqdet
