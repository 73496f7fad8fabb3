// Tensor statistics for the training summaries (sqdet_tensor_stats_many, include/sqdet.h): count, non-finite count, zero count,
// min, max, sum, sum of squares and a histogram over a caller-supplied edge table, for MANY segments of one buffer in one launch
// (+ one small finishing launch).  Replaces the per-variable tf.summary.histogram / zero_fraction / reduce_mean / reduce_max /
// reduce_min ops of nn_skeleton.py:353-358,736-755: a whole flat parameter or gradient bucket, or one activation, is one call.
//
// Work split.  A segment is cut into chunks of CHUNK_VECS 16-byte vectors; the chunks of all segments form one list that the
// workgroups walk with a stride of the grid, so a 38 M-element activation spreads over every workgroup and a 16-element bias is
// one chunk of one workgroup.  The 16-byte-aligned body of a segment is read with 16-byte loads, the unaligned head and the
// tail (fewer than one vector each) by a few lanes of the segment's first chunk.  Only [offset, offset + count) is read.
//
// Determinism.  sum and sumsq are float64 and never touch a float atomic: a thread adds its elements in index order, a workgroup
// reduces its threads in a fixed tree, writes ONE partial per (segment, workgroup) into the workspace, and the finishing launch
// adds the partials in workgroup order.  The element -> thread map depends only on the segment table and the grid, so two calls
// on the same data give the same bits.  Everything else is an integer (or a min / max through an order-preserving integer key)
// and goes through LDS and global integer atomics, whose result does not depend on the order.
//
// Binning is by float32 comparison only: the index of x is the number of edges <= x (np.searchsorted(edges, x, side="right")),
// found by binary search in an LDS copy of the table.  Zeros skip the search and the LDS atomic (a ReLU output is half zeros, all
// of one bin): they are counted in a register and added to the bin of 0.0f when the workgroup leaves the segment.
#include "common.h"

namespace sqdet {
namespace {

constexpr int THREADS = 256;
constexpr int VECS_PER_THREAD = 4;
constexpr int CHUNK_VECS = THREADS * VECS_PER_THREAD;      // 16 KiB per chunk
constexpr int MAX_BINS = 1024;
constexpr int MAX_GRID = 2048;

// record layout (include/sqdet.h): int64 count, nonfinite, zeros; float min, max; double sum, sumsq; int64 under, hist[n_bins], over
constexpr size_t REC_HEAD = 48;
inline __host__ __device__ size_t rec_bytes(int n_bins) { return REC_HEAD + 8 * (size_t)(n_bins + 2); }

struct StatsArgs {
  const void* base;
  int64_t base_count;
  const int64_t* offsets;
  const int64_t* counts;
  int n_segments;
  const float* edges;
  int n_bins;
  unsigned char* records;
  double* partial;          // [n_segments][grid][2]
  unsigned int* minmax;     // [n_segments][2]: atomicMax keys of -min and max, 0 = no finite element
};

// Monotone map float -> uint32 with every finite value above 0 (0 stays free as "nothing seen").
__device__ inline unsigned int order_key(float x) {
  const unsigned int b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float key_value(unsigned int k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

struct Acc {
  double sum, sumsq;
  float mn, mx;
  unsigned int nonfinite, zeros;
  __device__ void reset() {
    sum = 0.0; sumsq = 0.0;
    mn = __uint_as_float(0x7f800000u); mx = __uint_as_float(0xff800000u);
    nonfinite = 0; zeros = 0;
  }
};

__device__ inline void take(float x, Acc& a, const float* s_edges, unsigned int* s_cnt, int n_edges) {
  if ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) {      // NaN, +-inf
    ++a.nonfinite;
    return;
  }
  a.mn = x < a.mn ? x : a.mn;
  a.mx = x > a.mx ? x : a.mx;
  const double xd = (double)x;
  a.sum += xd;
  a.sumsq += xd * xd;          // a float32 square is exact in float64
  if (x == 0.0f) {
    ++a.zeros;
    return;
  }
  int lo = 0, hi = n_edges;    // number of edges <= x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s_edges[mid] <= x) lo = mid + 1; else hi = mid;
  }
  atomicAdd(&s_cnt[lo], 1u);
}

template <typename T> struct Vec;
template <> struct Vec<float> { typedef f32x4 V; static constexpr int N = 4; };
template <> struct Vec<f16> { typedef f16x8 V; static constexpr int N = 8; };

// A segment the kernel may read: inside the buffer.  (The table lives on the device, so the host cannot check it.)
__device__ inline bool segment_ok(int64_t off, int64_t cnt, int64_t base_count) {
  return off >= 0 && cnt >= 0 && off <= base_count && cnt <= base_count - off;
}

template <typename T>
__device__ inline int64_t segment_chunks(const T* base, int64_t off, int64_t cnt, int64_t base_count) {
  if (!segment_ok(off, cnt, base_count) || cnt == 0) return 0;
  constexpr int N = Vec<T>::N;
  const uintptr_t addr = reinterpret_cast<uintptr_t>(base + off);
  int64_t head = (int64_t)(((16 - (addr & 15)) & 15) / sizeof(T));
  if (head > cnt) head = cnt;
  const int64_t nv = (cnt - head) / N;
  const int64_t c = (nv + CHUNK_VECS - 1) / CHUNK_VECS;
  return c > 0 ? c : 1;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void stats_kernel(StatsArgs a) {
  typedef typename Vec<T>::V V;
  constexpr int N = Vec<T>::N;
  __shared__ float s_edges[MAX_BINS + 1];
  __shared__ unsigned int s_cnt[MAX_BINS + 2 + 2];      // index = number of edges <= x; then nonfinite, zeros
  __shared__ double s_red[2][THREADS / 64];
  __shared__ unsigned int s_mm[2];
  const int tid = threadIdx.x;
  const int n_edges = a.n_bins + 1, n_cnt = a.n_bins + 2;
  for (int i = tid; i < n_edges; i += THREADS) s_edges[i] = a.edges[i];
  for (int i = tid; i < n_cnt + 2; i += THREADS) s_cnt[i] = 0;
  if (tid < 2) s_mm[tid] = 0;
  __syncthreads();
  int zero_idx = 0;                                      // bin index of 0.0f
  {
    int lo = 0, hi = n_edges;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_edges[mid] <= 0.0f) lo = mid + 1; else hi = mid;
    }
    zero_idx = lo;
  }
  const T* base = reinterpret_cast<const T*>(a.base);
  Acc acc;
  acc.reset();

  // leaves segment `s`: the workgroup's share of it goes out -- one float64 partial pair, one key pair, the non-zero counters
  auto flush = [&](int s) {
    double v0 = acc.sum, v1 = acc.sumsq;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      v0 += __shfl_down(v0, d, 64);
      v1 += __shfl_down(v1, d, 64);
    }
    if ((tid & 63) == 0) {
      s_red[0][tid >> 6] = v0;
      s_red[1][tid >> 6] = v1;
    }
    if (acc.nonfinite) atomicAdd(&s_cnt[n_cnt], acc.nonfinite);
    if (acc.zeros) atomicAdd(&s_cnt[n_cnt + 1], acc.zeros);
    if (acc.mx >= acc.mn) {                              // saw a finite element
      atomicMax(&s_mm[0], order_key(-acc.mn));
      atomicMax(&s_mm[1], order_key(acc.mx));
    }
    __syncthreads();
    unsigned char* rec = a.records + (size_t)s * rec_bytes(a.n_bins);
    unsigned long long* r64 = reinterpret_cast<unsigned long long*>(rec);
    if (tid == 0) {
      double t0 = s_red[0][0], t1 = s_red[1][0];
      for (int w = 1; w < THREADS / 64; ++w) {
        t0 += s_red[0][w];
        t1 += s_red[1][w];
      }
      double* p = a.partial + ((size_t)s * gridDim.x + blockIdx.x) * 2;
      p[0] = t0;
      p[1] = t1;
      if (s_mm[0]) atomicMax(&a.minmax[2 * s], s_mm[0]);
      if (s_mm[1]) atomicMax(&a.minmax[2 * s + 1], s_mm[1]);
      if (s_cnt[n_cnt]) atomicAdd(&r64[1], (unsigned long long)s_cnt[n_cnt]);
      if (s_cnt[n_cnt + 1]) atomicAdd(&r64[2], (unsigned long long)s_cnt[n_cnt + 1]);
    }
    for (int i = tid; i < n_cnt; i += THREADS) {
      unsigned int c = s_cnt[i];
      if (i == zero_idx) c += s_cnt[n_cnt + 1];
      if (c) atomicAdd(&r64[REC_HEAD / 8 + i], (unsigned long long)c);
    }
    __syncthreads();
    for (int i = tid; i < n_cnt + 2; i += THREADS) s_cnt[i] = 0;
    if (tid < 2) s_mm[tid] = 0;
    acc.reset();
    __syncthreads();
  };

  // the workgroup's chunks g = blockIdx.x, + gridDim.x, ...: g only grows, so the segment cursor only moves forward
  int seg = 0, open = -1;
  int64_t seg_first = 0;                                 // global index of segment seg's first chunk
  int64_t seg_n = a.n_segments > 0 ? segment_chunks(base, a.offsets[0], a.counts[0], a.base_count) : 0;
  for (int64_t g = blockIdx.x;; g += gridDim.x) {
    while (seg < a.n_segments && g >= seg_first + seg_n) {
      seg_first += seg_n;
      ++seg;
      seg_n = seg < a.n_segments ? segment_chunks(base, a.offsets[seg], a.counts[seg], a.base_count) : 0;
    }
    if (seg >= a.n_segments) break;
    if (open != seg) {
      if (open >= 0) flush(open);
      open = seg;
    }
    const int64_t off = a.offsets[seg], cnt = a.counts[seg];
    const T* p = base + off;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    int64_t head = (int64_t)(((16 - (addr & 15)) & 15) / sizeof(T));
    if (head > cnt) head = cnt;
    const int64_t nv = (cnt - head) / N;
    const int64_t local = g - seg_first;
    if (local == 0) {                                    // the scalar head and tail ride on the first chunk
      const int64_t tail0 = head + nv * N;
      if (tid < head) take((float)p[tid], acc, s_edges, s_cnt, n_edges);
      if (tid >= 32 && tail0 + (tid - 32) < cnt) take((float)p[tail0 + (tid - 32)], acc, s_edges, s_cnt, n_edges);
    }
    const V* pv = reinterpret_cast<const V*>(p + head);
    const int64_t v0 = local * CHUNK_VECS + tid;
    V v[VECS_PER_THREAD];
#pragma unroll
    for (int j = 0; j < VECS_PER_THREAD; ++j)
      if (v0 + j * THREADS < nv) v[j] = pv[v0 + j * THREADS];
#pragma unroll
    for (int j = 0; j < VECS_PER_THREAD; ++j)
      if (v0 + j * THREADS < nv) {
#pragma unroll
        for (int e = 0; e < N; ++e) take((float)v[j][e], acc, s_edges, s_cnt, n_edges);
      }
  }
  if (open >= 0) flush(open);
}

// One workgroup per segment: the partials in workgroup order, then count / min / max / sum / sumsq into the record.
__global__ __launch_bounds__(THREADS) void stats_finish_kernel(StatsArgs a, int grid) {
  __shared__ double s_red[2][THREADS];
  const int s = blockIdx.x, tid = threadIdx.x;
  const double* p = a.partial + (size_t)s * grid * 2;
  const int per = (grid + THREADS - 1) / THREADS;
  double t0 = 0.0, t1 = 0.0;
  for (int i = tid * per; i < (tid + 1) * per && i < grid; ++i) {
    t0 += p[2 * i];
    t1 += p[2 * i + 1];
  }
  s_red[0][tid] = t0;
  s_red[1][tid] = t1;
  __syncthreads();
  for (int d = THREADS / 2; d > 0; d >>= 1) {
    if (tid < d) {
      s_red[0][tid] += s_red[0][tid + d];
      s_red[1][tid] += s_red[1][tid + d];
    }
    __syncthreads();
  }
  if (tid == 0) {
    unsigned char* rec = a.records + (size_t)s * rec_bytes(a.n_bins);
    const int64_t off = a.offsets[s], cnt = a.counts[s];
    reinterpret_cast<int64_t*>(rec)[0] = segment_ok(off, cnt, a.base_count) ? cnt : -1;      // -1: a segment outside the buffer, not read
    const unsigned int kmin = a.minmax[2 * s], kmax = a.minmax[2 * s + 1];
    float* mm = reinterpret_cast<float*>(rec + 24);
    mm[0] = kmin ? -key_value(kmin) : __uint_as_float(0x7f800000u);
    mm[1] = kmax ? key_value(kmax) : __uint_as_float(0xff800000u);
    double* sums = reinterpret_cast<double*>(rec + 32);
    sums[0] = s_red[0][0];
    sums[1] = s_red[1][0];
  }
}

int stats_grid() {
  const int g = cu_count() * 8;
  return g < MAX_GRID ? g : MAX_GRID;
}

}  // namespace
}  // namespace sqdet

using namespace sqdet;

extern "C" size_t sqdet_tensor_stats_record_bytes(int n_bins) {
  return n_bins >= 1 && n_bins <= MAX_BINS ? rec_bytes(n_bins) : 0;
}

extern "C" size_t sqdet_tensor_stats_workspace_bytes(int n_segments, int n_bins) {
  if (n_segments <= 0 || n_bins < 1 || n_bins > MAX_BINS) return 0;
  // (sized for the largest grid the launcher ever uses, so the answer needs no device)
  return (size_t)n_segments * MAX_GRID * 2 * sizeof(double) + (size_t)n_segments * 2 * sizeof(unsigned int);
}

extern "C" int sqdet_tensor_stats_many(const void* base, int64_t base_count, const int64_t* offsets_dev, const int64_t* counts_dev,
                                       int n_segments, const float* edges_dev, int n_bins, void* records_dev, void* workspace,
                                       int dtype, sqdet_stream_t stream) {
  SQDET_REQUIRE(dtype == SQDET_F16 || dtype == SQDET_F32, "tensor_stats: bad dtype");
  SQDET_REQUIRE(base && offsets_dev && counts_dev && edges_dev && records_dev && workspace, "tensor_stats: null pointer");
  SQDET_REQUIRE(n_segments > 0 && base_count >= 0, "tensor_stats: bad segment count or buffer size");
  SQDET_REQUIRE(n_bins >= 1 && n_bins <= MAX_BINS, "tensor_stats: n_bins must be in [1, %d]", MAX_BINS);
  SQDET_REQUIRE(reinterpret_cast<uintptr_t>(base) % dtype_size(dtype) == 0 && reinterpret_cast<uintptr_t>(records_dev) % 8 == 0 &&
                reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "tensor_stats: misaligned pointer");
  const int grid = stats_grid();
  StatsArgs a;
  a.base = base;
  a.base_count = base_count;
  a.offsets = offsets_dev;
  a.counts = counts_dev;
  a.n_segments = n_segments;
  a.edges = edges_dev;
  a.n_bins = n_bins;
  a.records = static_cast<unsigned char*>(records_dev);
  a.partial = static_cast<double*>(workspace);
  a.minmax = reinterpret_cast<unsigned int*>(static_cast<unsigned char*>(workspace) + (size_t)n_segments * MAX_GRID * 2 * sizeof(double));
  hipStream_t st = as_stream(stream);
  SQDET_CHECK_HIP(hipMemsetAsync(records_dev, 0, (size_t)n_segments * rec_bytes(n_bins), st));
  // (the partials are laid out [segment][grid], grid <= MAX_GRID: only that prefix is used and zeroed)
  SQDET_CHECK_HIP(hipMemsetAsync(a.partial, 0, (size_t)n_segments * grid * 2 * sizeof(double), st));
  SQDET_CHECK_HIP(hipMemsetAsync(a.minmax, 0, (size_t)n_segments * 2 * sizeof(unsigned int), st));
  if (dtype == SQDET_F16)
    hipLaunchKernelGGL(stats_kernel<f16>, dim3(grid), dim3(THREADS), 0, st, a);
  else
    hipLaunchKernelGGL(stats_kernel<float>, dim3(grid), dim3(THREADS), 0, st, a);
  SQDET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(stats_finish_kernel, dim3(n_segments), dim3(THREADS), 0, st, a, grid);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}
