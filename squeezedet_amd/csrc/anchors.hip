// Anchor shapes for a dataset, on the GPU: Lloyd's k-means over box shapes under the IoU distance, and a report of how an
// anchor grid covers a set of ground-truth boxes.  OURS for the fitting: the reference ships fixed shapes only
// (config/kitti_squeezeDet_config.py:45-79).  The coverage figures are what the reference's mc.DEBUG_MODE branch of
// imdb.read_batch accumulates (dataset/imdb.py:135-139, 203-215, 241-246) from util.batch_iou (utils/util.py:32-54), per object
// instead of as five printed totals.
//
// k-means.  The distance of two shapes is 1 - IoU of the two boxes on a common centre, in double, in this order:
//   inter = min(w, cw) * min(h, ch);  iou = inter / (w*h + cw*ch - inter)
// Every restart r runs at once (blockIdx.y).  One iteration is two launches, and nothing returns to the host between them:
//   kmeans_assign_kernel   (ceil(n/1024), R) x 256: the restart's centroids in LDS; each thread takes 4 boxes (coalesced, 256
//       apart), gives each to the centroid of highest IoU (lowest index on a tie, np.argmax) and notes whether that changed;
//       then, per centroid, the workgroup's sum of member widths, heights and its member count: the thread's 4 boxes in
//       order, a wave64 shuffle tree, the 4 waves in order through LDS -> one partial per (restart, workgroup, centroid);
//   kmeans_update_kernel   R x 256: per centroid one wave adds the workgroups' partials (lane l takes workgroups l, l+64, ..
//       in order, then the shuffle tree) and divides sum by count; a centroid without members keeps its value; the first
//       iteration in which no workgroup saw a change is recorded.
// Past convergence an iteration reproduces the fixed point bit for bit (same members, same order), so all max_iter iterations
// are enqueued and none needs the host.  Then kmeans_iou_kernel / kmeans_finish_kernel take the mean IoU the same way.  Every
// floating-point sum has a fixed shape that depends on n only: no float atomics, two calls are bitwise equal.
//
// Coverage.  One workgroup per ground-truth box, as labels_best_kernel: 256 threads stride over the A anchors, each keeps its
// best (IoU, index), a wave64 shuffle reduction and 4 candidates through LDS; the maximum is order-free and the FIRST index
// attains it (np.argmax).  Thread 0 also takes the IoU with the anchor sqdet_build_labels gave the box.
#include <limits.h>
#include "common.h"

namespace sqdet {

constexpr int KM_THREADS = 256;
constexpr int KM_PER_THREAD = 4;
constexpr int KM_CHUNK = KM_THREADS * KM_PER_THREAD;   // boxes per workgroup
constexpr int KM_WAVES = KM_THREADS / 64;

__device__ __forceinline__ double shape_iou(double w, double h, double cw, double ch) {
  const double inter = fmin(w, cw) * fmin(h, ch);
  return inter / (w * h + cw * ch - inter);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  return v;                                              // lane 0 holds the tree's root
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  return v;
}

// Layout of the workspace for (n, k, R): doubles first.
struct KmWorkspace {
  double* psum;   // [R, nblk, k, 2]  per-workgroup sums of member (w, h)
  double* piou;   // [R, nblk]        per-workgroup sums of IoU
  int* pcnt;      // [R, nblk, k]     per-workgroup member counts
  int* pchg;      // [R, nblk]        1: an assignment of this workgroup changed
};
__host__ __device__ inline int km_blocks(int n) { return (n + KM_CHUNK - 1) / KM_CHUNK; }
inline size_t km_workspace_bytes(int n, int k, int R) {
  const size_t nb = (size_t)km_blocks(n) * R;
  return nb * k * 2 * sizeof(double) + nb * sizeof(double) + nb * k * sizeof(int) + nb * sizeof(int);
}
inline KmWorkspace km_workspace(void* ws, int n, int k, int R) {
  const size_t nb = (size_t)km_blocks(n) * R;
  KmWorkspace w;
  w.psum = (double*)ws;
  w.piou = w.psum + nb * k * 2;
  w.pcnt = (int*)(w.piou + nb);
  w.pchg = w.pcnt + nb * k;
  return w;
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(const double* __restrict__ wh, const double* __restrict__ cent,
                                                                   int* __restrict__ assign, int* __restrict__ iters,
                                                                   double* __restrict__ psum, int* __restrict__ pcnt,
                                                                   int* __restrict__ pchg, int n, int k, int max_iter, int first) {
  __shared__ double s_cw[SQDET_ANCHOR_KMEANS_MAX_K], s_ch[SQDET_ANCHOR_KMEANS_MAX_K];
  __shared__ double s_rw[KM_WAVES][SQDET_ANCHOR_KMEANS_MAX_K], s_rh[KM_WAVES][SQDET_ANCHOR_KMEANS_MAX_K];
  __shared__ int s_rc[KM_WAVES][SQDET_ANCHOR_KMEANS_MAX_K];
  __shared__ int s_chg[KM_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = blockIdx.x, nblk = gridDim.x, r = blockIdx.y;
  if (tid < k) {
    s_cw[tid] = cent[((size_t)r * k + tid) * 2];
    s_ch[tid] = cent[((size_t)r * k + tid) * 2 + 1];
  }
  if (first && blk == 0 && tid == 0) iters[r] = max_iter;
  __syncthreads();
  double w[KM_PER_THREAD], h[KM_PER_THREAD];
  int a[KM_PER_THREAD];
  int changed = 0;
#pragma unroll
  for (int j = 0; j < KM_PER_THREAD; ++j) {
    const int i = blk * KM_CHUNK + j * KM_THREADS + tid;   // n <= INT_MAX and blk * KM_CHUNK < n
    w[j] = 0.0; h[j] = 0.0; a[j] = -1;
    if (i < n) {
      w[j] = wh[(size_t)i * 2];
      h[j] = wh[(size_t)i * 2 + 1];
      double best = shape_iou(w[j], h[j], s_cw[0], s_ch[0]);
      int bi = 0;
      for (int c = 1; c < k; ++c) {
        const double v = shape_iou(w[j], h[j], s_cw[c], s_ch[c]);
        if (v > best) { best = v; bi = c; }                // strict: the lowest index keeps a tie
      }
      a[j] = bi;
      const size_t o = (size_t)r * n + i;
      if (first || assign[o] != bi) changed = 1;
      assign[o] = bi;
    }
  }
  for (int c = 0; c < k; ++c) {
    double sw = 0.0, sh = 0.0;
    int cn = 0;
    bool any = false;
#pragma unroll
    for (int j = 0; j < KM_PER_THREAD; ++j) {
      const bool m = a[j] == c;
      sw += m ? w[j] : 0.0;                                // adding 0.0 is exact: the sum keeps its shape whoever is a member
      sh += m ? h[j] : 0.0;
      cn += m ? 1 : 0;
      any |= m;
    }
    if (__any(any)) {                                      // wave-uniform; a wave without members contributes exact zeros
      sw = wave_sum(sw);
      sh = wave_sum(sh);
      cn = wave_sum(cn);
    }
    if (lane == 0) { s_rw[wave][c] = sw; s_rh[wave][c] = sh; s_rc[wave][c] = cn; }
  }
  const int chg = __any(changed);
  if (lane == 0) s_chg[wave] = chg ? 1 : 0;
  __syncthreads();
  const size_t pb = (size_t)r * nblk + blk;
  if (tid < k) {
    double sw = s_rw[0][tid], sh = s_rh[0][tid];
    int cn = s_rc[0][tid];
#pragma unroll
    for (int v = 1; v < KM_WAVES; ++v) { sw += s_rw[v][tid]; sh += s_rh[v][tid]; cn += s_rc[v][tid]; }
    psum[(pb * k + tid) * 2] = sw;
    psum[(pb * k + tid) * 2 + 1] = sh;
    pcnt[pb * k + tid] = cn;
  }
  if (tid == 0) {
    int cg = 0;
#pragma unroll
    for (int v = 0; v < KM_WAVES; ++v) cg |= s_chg[v];
    pchg[pb] = cg;
  }
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_update_kernel(double* __restrict__ cent, int* __restrict__ counts,
                                                                   int* __restrict__ iters, const double* __restrict__ psum,
                                                                   const int* __restrict__ pcnt, const int* __restrict__ pchg,
                                                                   int k, int nblk, int max_iter, int it) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
  const size_t pb = (size_t)r * nblk;
  for (int c = wave; c < k; c += KM_WAVES) {
    double sw = 0.0, sh = 0.0;
    int cn = 0;
    for (int b = lane; b < nblk; b += 64) {
      sw += psum[((pb + b) * k + c) * 2];
      sh += psum[((pb + b) * k + c) * 2 + 1];
      cn += pcnt[(pb + b) * k + c];
    }
    sw = wave_sum(sw);
    sh = wave_sum(sh);
    cn = wave_sum(cn);
    if (lane == 0) {
      counts[(size_t)r * k + c] = cn;
      if (cn > 0) {
        cent[((size_t)r * k + c) * 2] = sw / (double)cn;
        cent[((size_t)r * k + c) * 2 + 1] = sh / (double)cn;
      }
    }
  }
  if (wave == 0) {
    int cg = 0;
    for (int b = lane; b < nblk; b += 64) cg |= pchg[pb + b];
    cg = __any(cg);
    if (lane == 0 && !cg && iters[r] == max_iter) iters[r] = it;
  }
}

// Sum of IoU(box, the centroid it is assigned to) per workgroup.
__global__ __launch_bounds__(KM_THREADS) void kmeans_iou_kernel(const double* __restrict__ wh, const double* __restrict__ cent,
                                                                const int* __restrict__ assign, double* __restrict__ piou, int n,
                                                                int k) {
  __shared__ double s_cw[SQDET_ANCHOR_KMEANS_MAX_K], s_ch[SQDET_ANCHOR_KMEANS_MAX_K];
  __shared__ double s_r[KM_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = blockIdx.x, nblk = gridDim.x, r = blockIdx.y;
  if (tid < k) {
    s_cw[tid] = cent[((size_t)r * k + tid) * 2];
    s_ch[tid] = cent[((size_t)r * k + tid) * 2 + 1];
  }
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < KM_PER_THREAD; ++j) {
    const int i = blk * KM_CHUNK + j * KM_THREADS + tid;
    double v = 0.0;
    if (i < n) {
      int c = assign[(size_t)r * n + i];
      c = c < 0 ? 0 : (c >= k ? k - 1 : c);                // (always in range: written by kmeans_assign_kernel)
      v = shape_iou(wh[(size_t)i * 2], wh[(size_t)i * 2 + 1], s_cw[c], s_ch[c]);
    }
    s += v;
  }
  s = wave_sum(s);
  if (lane == 0) s_r[wave] = s;
  __syncthreads();
  if (tid == 0) {
    double t = s_r[0];
#pragma unroll
    for (int v = 1; v < KM_WAVES; ++v) t += s_r[v];
    piou[(size_t)r * nblk + blk] = t;
  }
}

__global__ __launch_bounds__(64) void kmeans_finish_kernel(const double* __restrict__ piou, double* __restrict__ mean_iou, int n,
                                                           int nblk) {
  const int lane = threadIdx.x, r = blockIdx.x;
  double s = 0.0;
  for (int b = lane; b < nblk; b += 64) s += piou[(size_t)r * nblk + b];
  s = wave_sum(s);
  if (lane == 0) mean_iou[r] = s / (double)n;
}

// --------------------------------------------------------------------------------------------------------- coverage --
struct Cov {
  double v;
  int idx;
};
// a wins over b: larger IoU, the LOWER index on a tie (np.argmax's first maximum)
__device__ __forceinline__ bool cov_better(const Cov& a, const Cov& b) { return a.v > b.v || (a.v == b.v && a.idx < b.idx); }

// util.batch_iou(anchors, box) for one anchor, in the reference's operation order
__device__ __forceinline__ double anchor_iou(const double* __restrict__ an, double gx, double gy, double gw, double gh) {
  const double ax = an[0], ay = an[1], aw = an[2], ah = an[3];
  double lr = fmin(ax + 0.5 * aw, gx + 0.5 * gw) - fmax(ax - 0.5 * aw, gx - 0.5 * gw);
  lr = lr > 0.0 ? lr : 0.0;
  double tb = fmin(ay + 0.5 * ah, gy + 0.5 * gh) - fmax(ay - 0.5 * ah, gy - 0.5 * gh);
  tb = tb > 0.0 ? tb : 0.0;
  const double inter = lr * tb;
  return inter / (aw * ah + gw * gh - inter);
}

__global__ __launch_bounds__(256) void anchor_coverage_kernel(const double* __restrict__ anchors, const double* __restrict__ gt,
                                                              const int* __restrict__ gt_count, const int* __restrict__ anchor_index,
                                                              double* __restrict__ best_iou, int* __restrict__ best_index,
                                                              double* __restrict__ claimed_iou, int A, int M) {
  __shared__ Cov red[4];
  const size_t o = blockIdx.x;                             // b * M + i
  const int b = (int)(o / (size_t)M), i = (int)(o % (size_t)M);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = gt_count[b];
  if (n > M) n = M;
  if (i >= n) {                                            // workgroup-uniform
    if (tid == 0) { best_iou[o] = 0.0; best_index[o] = -1; claimed_iou[o] = 0.0; }
    return;
  }
  const double gx = gt[o * 4], gy = gt[o * 4 + 1], gw = gt[o * 4 + 2], gh = gt[o * 4 + 3];
  Cov c;
  c.v = -1.0; c.idx = INT_MAX;
  for (int a = tid; a < A; a += 256) {
    Cov t;
    t.v = anchor_iou(anchors + (size_t)a * 4, gx, gy, gw, gh);
    t.idx = a;
    if (cov_better(t, c)) c = t;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Cov t;
    t.v = __shfl_down(c.v, off);
    t.idx = __shfl_down(c.idx, off);
    if (cov_better(t, c)) c = t;
  }
  if (lane == 0) red[wave] = c;
  __syncthreads();
  if (tid == 0) {
    Cov m = red[0];
#pragma unroll
    for (int v = 1; v < 4; ++v)
      if (cov_better(red[v], m)) m = red[v];
    if (m.idx == INT_MAX) { m.v = 0.0; m.idx = 0; }        // (no comparable IoU at all: NaN boxes, which the callers reject)
    best_iou[o] = m.v;
    best_index[o] = m.idx;
    double cl = 0.0;
    if (anchor_index) {
      const int a = anchor_index[o];
      if (a >= 0 && a < A) cl = anchor_iou(anchors + (size_t)a * 4, gx, gy, gw, gh);
    }
    claimed_iou[o] = cl;
  }
}

}  // namespace sqdet

extern "C" size_t sqdet_anchor_kmeans_workspace_bytes(int n, int k, int restarts) {
  if (n < 1 || k < 1 || restarts < 1 || k > SQDET_ANCHOR_KMEANS_MAX_K || restarts > SQDET_ANCHOR_KMEANS_MAX_RESTARTS) return 0;
  return sqdet::km_workspace_bytes(n, k, restarts);
}

extern "C" int sqdet_anchor_kmeans(const double* wh, double* centroids, int* assign, int* counts, double* mean_iou, int* iters,
                                   void* workspace, int n, int k, int restarts, int max_iter, sqdet_stream_t stream) {
  using namespace sqdet;
  SQDET_REQUIRE(wh && centroids && assign && counts && mean_iou && iters && workspace, "anchor_kmeans: null pointer");
  SQDET_REQUIRE(n >= 1 && k >= 1 && restarts >= 1 && max_iter >= 1, "anchor_kmeans: bad dims (n %d, k %d, restarts %d, max_iter %d)",
                n, k, restarts, max_iter);
  SQDET_UNSUPPORTED(k > SQDET_ANCHOR_KMEANS_MAX_K, "anchor_kmeans: k %d over the limit of %d", k, SQDET_ANCHOR_KMEANS_MAX_K);
  SQDET_UNSUPPORTED(restarts > SQDET_ANCHOR_KMEANS_MAX_RESTARTS, "anchor_kmeans: %d restarts over the limit of %d", restarts,
                    SQDET_ANCHOR_KMEANS_MAX_RESTARTS);
  hipStream_t st = as_stream(stream);
  const int nblk = km_blocks(n);
  const KmWorkspace w = km_workspace(workspace, n, k, restarts);
  const dim3 grid((unsigned)nblk, (unsigned)restarts);
  for (int it = 0; it < max_iter; ++it) {
    hipLaunchKernelGGL(kmeans_assign_kernel, grid, dim3(KM_THREADS), 0, st, wh, centroids, assign, iters, w.psum, w.pcnt, w.pchg, n, k,
                       max_iter, it == 0 ? 1 : 0);
    hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)restarts), dim3(KM_THREADS), 0, st, centroids, counts, iters, w.psum, w.pcnt,
                       w.pchg, k, nblk, max_iter, it);
  }
  hipLaunchKernelGGL(kmeans_iou_kernel, grid, dim3(KM_THREADS), 0, st, wh, centroids, assign, w.piou, n, k);
  hipLaunchKernelGGL(kmeans_finish_kernel, dim3((unsigned)restarts), dim3(64), 0, st, w.piou, mean_iou, n, nblk);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" int sqdet_anchor_coverage(const double* anchors_f64, const double* gt_boxes_f64, const int* gt_counts,
                                     const int* anchor_index, double* best_iou, int* best_index, double* claimed_iou, int batch,
                                     int num_anchors, int max_objects, sqdet_stream_t stream) {
  using namespace sqdet;
  SQDET_REQUIRE(anchors_f64 && gt_boxes_f64 && gt_counts && best_iou && best_index && claimed_iou, "anchor_coverage: null pointer");
  SQDET_REQUIRE(batch > 0 && num_anchors > 0 && max_objects > 0, "anchor_coverage: bad dims");
  SQDET_UNSUPPORTED((size_t)batch * max_objects > (size_t)INT_MAX, "anchor_coverage: more than 2^31 - 1 table entries");
  hipLaunchKernelGGL(anchor_coverage_kernel, dim3((unsigned)((size_t)batch * max_objects)), dim3(256), 0, as_stream(stream), anchors_f64,
                     gt_boxes_f64, gt_counts, anchor_index, best_iou, best_index, claimed_iou, num_anchors, max_objects);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}
